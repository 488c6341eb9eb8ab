"""The trainable SEED-Encoder without a GPU: every refusal of ance_pack_tokens_by_id (include/ance_amd.h) -- on the host, before any
launch: the device pointers are fake and never dereferenced -- held to its whole message ("<entry point>: invalid argument
(<reason>)", csrc/pack_rows.hip behind common.h's refuse()); the binding's struct layout against the header; the refusals of
ance_amd.model.SEEDEncoderDot_NLL_LN's constructor; its parameter names against the reference's own (tests/golden/seed_step.json);
strict loading, and the round trip through reference_state_dict() into ance_amd.encoder.seed_state_dict."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import seed_util
from ance_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000
FN = "ance_pack_tokens_by_id"
VOCAB, MAX_POS = seed_util.SEED_VOCAB, 514

NULL = "null pointer"
ALIGN4 = "alignment: an integer array is not 4-byte aligned"
ALIGN8 = "alignment: d_dropped is not 8-byte aligned"
N_SEQ = "n_seq outside 1 .. 65535"
LENGTH = "L outside 1 .. 512"
ROWS = "rows < 1"
TABLE = "an empty table"
PAD = "padding_idx outside 0 .. vocab - 1"
POINTERS = ("ids", "d_seq_len", "d_seq_off", "d_seq_kept", "d_dropped", "packed_ids", "packed_positions")


def _args(**kw):
    a = _lib.AncePackByIdArgs(ids=FAKE, d_seq_len=FAKE, d_seq_off=FAKE, d_seq_kept=FAKE, d_dropped=FAKE, packed_ids=FAKE,
                              packed_positions=FAKE, n_seq=3, L=40, rows=90, padding_idx=1, vocab=VOCAB, max_pos=MAX_POS)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_pack_by_id_refuses_before_any_launch():
    L = _lib.lib()

    def refused(why, **kw):
        a = _args(**kw)
        rc, msg = L.ance_pack_tokens_by_id(ctypes.byref(a), None), L.ance_last_error().decode()
        assert rc == _lib.ANCE_E_INVALID and msg == "%s: invalid argument (%s)" % (FN, why), (why, kw, rc, msg)

    rc, msg = L.ance_pack_tokens_by_id(None, None), L.ance_last_error().decode()
    assert rc == _lib.ANCE_E_INVALID and msg == "%s: invalid argument (%s)" % (FN, NULL)
    for f in POINTERS:
        refused(NULL, **{f: None})
    for f in POINTERS:
        if f != "d_dropped":
            for off in (1, 2, 3):
                refused(ALIGN4, **{f: FAKE + off})
    for off in (1, 4, 12):
        refused(ALIGN8, d_dropped=FAKE + off)
    for n in (0, -1, 65536):
        refused(N_SEQ, n_seq=n)
    for n in (0, -1, 513):
        refused(LENGTH, L=n)
    for n in (0, -5):
        refused(ROWS, rows=n)
    refused(TABLE, vocab=0)
    refused(TABLE, max_pos=0)
    for p in (-1, -2, VOCAB, VOCAB + 1):
        refused(PAD, padding_idx=p)
    # the order: the sizes before the pointers, so a refusal never depends on an address
    refused(N_SEQ, n_seq=0, ids=None)
    refused(PAD, padding_idx=-1, d_dropped=FAKE + 4)


def test_header_and_binding_agree(tmp_path):
    """The entry point is declared, exported and bound; sizeof and every offsetof of AncePackByIdArgs, from a C program compiled
    against include/ance_amd.h; the ABI version is still 7 (the change is additive)."""
    hdr = open(os.path.join(ROOT, "include", "ance_amd.h")).read()
    assert "int ance_pack_tokens_by_id(const AncePackByIdArgs *args, void *stream);" in hdr
    assert "#define ANCE_ABI_VERSION 7" in hdr and _lib.ABI_VERSION == 7 and _lib.lib().ance_abi_version() == 7
    res, argtypes = _lib.SYMBOLS[FN]
    assert res is ctypes.c_int and argtypes == [ctypes.POINTER(_lib.AncePackByIdArgs), ctypes.c_void_p]
    fields = [f for f, _ in _lib.AncePackByIdArgs._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "ance_amd.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(AncePackByIdArgs));']
    lines += ['printf("%s %%zu\\n", offsetof(AncePackByIdArgs, %s));' % (f, f) for f in fields]
    lines.append("return 0; }")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if subprocess.run(
        ["sh", "-c", "command -v %s" % c], capture_output=True).returncode == 0), None)
    assert cc is not None, "no C compiler"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(_lib.AncePackByIdArgs)
    for f in fields:
        assert int(got[f]) == getattr(_lib.AncePackByIdArgs, f).offset, f


def test_python_front_end_refuses_on_the_host():
    from ance_amd import packing
    with pytest.raises(_lib.AnceLibraryError, match="input_ids must be a CUDA"):
        packing.pack_tokens_by_id(torch.zeros(2, 4, dtype=torch.int64), 8, 1)
    assert packing.PackRule.of("seed", 1, VOCAB, MAX_POS) != packing.PackRule.of("roberta", 1, VOCAB, MAX_POS)


# ---------------------------------------------------------------------------------------------------------------- the model
class Config(object):
    """The reference's SEEDEncoderConfig by its attribute names and defaults."""

    def __init__(self, **kw):
        d = dict(pad_token_id=1, vocab_size=VOCAB, encoder_layers=2, encoder_embed_dim=768, encoder_ffn_embed_dim=3072,
                 encoder_attention_heads=12, dropout=0.1, attention_dropout=0.1, activation_dropout=0.0, encoder_layerdrop=0.0,
                 max_positions=512, activation_fn="gelu", quant_noise_pq=0.0, quant_noise_pq_block_size=8)
        d.update(kw)
        self.__dict__.update(d)


class ArgObj(object):
    use_mean = True


@pytest.mark.parametrize("setting,kw", [("activation_dropout", dict(activation_dropout=0.1)), ("encoder_layerdrop", dict(encoder_layerdrop=0.2)),
                                        ("quant_noise_pq", dict(quant_noise_pq=0.05)), ("activation_fn", dict(activation_fn="relu")),
                                        ("encoder_embed_dim", dict(encoder_embed_dim=1024, encoder_attention_heads=16,
                                                                   encoder_ffn_embed_dim=4096)),
                                        ("encoder_embed_dim", dict(encoder_attention_heads=8)),
                                        ("encoder_embed_dim", dict(encoder_ffn_embed_dim=4096))])
def test_constructor_refuses_by_name(setting, kw):
    from ance_amd.model import SEEDEncoderDot_NLL_LN
    with pytest.raises(_lib.AnceLibraryError, match=setting):
        SEEDEncoderDot_NLL_LN(Config(**kw))


def test_constructor_refuses_use_mean_and_takes_the_defaults():
    from ance_amd.model import SEEDEncoderDot_NLL_LN
    with pytest.raises(_lib.AnceLibraryError, match="use_mean"):
        SEEDEncoderDot_NLL_LN(Config(), ArgObj())
    with pytest.raises(_lib.AnceLibraryError, match="precision"):
        SEEDEncoderDot_NLL_LN(Config(), precision="fp16")
    m = SEEDEncoderDot_NLL_LN(Config(encoder_layers=1))
    enc = m.seed_encoder.encoder.sentence_encoder
    assert tuple(enc.embed_positions.weight.shape) == (514, 768) and enc.embed_tokens.padding_idx == 1
    assert enc.pack_rule == ("seed", 1, VOCAB, 514)
    assert m.towers() == (enc, enc)


def _sd(n_layers=2, seed=61):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in seed_util.det_seed_state_dict(seed, n_layers, 0.1).items()}


def test_parameter_names_are_the_references(golden_dir):
    """named_parameters() of a 2-layer model, in order, is the list the reference's own SEEDEncoderDot_NLL_LN gave the generator
    (its used parameters: classification_heads.* left out); state_dict() holds the same names and nothing else."""
    from ance_amd.model import SEEDEncoderDot_NLL_LN
    with open(os.path.join(golden_dir, "seed_step.json")) as f:
        want = json.load(f)["params"]
    m = SEEDEncoderDot_NLL_LN(Config())
    assert [n for n, _ in m.named_parameters()] == want
    assert list(m.state_dict()) == want                                    # the zero segment row is not persistent
    seg = dict(m.named_buffers())[seed_util.SRC + "no_segment"]
    assert tuple(seg.shape) == (1, 768) and not seg.any() and not seg.requires_grad
    # the reference's grouping no_decay = ["bias", "LayerNorm.weight"]: SEED's *_layer_norm.weight are decayed, as there
    decayed = [n for n in want if not any(nd in n for nd in ("bias", "LayerNorm.weight"))]
    assert seed_util.SRC + "emb_layer_norm.weight" in decayed and seed_util.SRC + "layers.1.final_layer_norm.weight" in decayed
    # the shared forward text reads the same modules under BertLayer's names; nothing is registered twice
    layer = m.seed_encoder.encoder.sentence_encoder.layers[1]
    assert layer.attention.self.key is layer.self_attn.k_proj and layer.output.LayerNorm is layer.final_layer_norm
    assert len(list(m.parameters())) == len(want)


def test_strict_load_and_set_aside():
    from ance_amd.model import SEEDEncoderDot_NLL_LN
    sd = _sd()
    m = SEEDEncoderDot_NLL_LN.from_state_dict(sd)
    assert len(m.seed_encoder.encoder.sentence_encoder.layers) == 2
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    heads = {"classification_heads.dense.weight": torch.ones(768, 768), "classification_heads.out_proj.bias": torch.zeros(2)}
    m = SEEDEncoderDot_NLL_LN(Config()).load_reference_state_dict(dict(sd, **heads))
    out = m.reference_state_dict()
    assert set(out) == set(sd) | set(heads) and all(torch.equal(out[k], v) for k, v in heads.items())
    assert not any(k.startswith("classification_heads.") for k in m.state_dict())
    short = dict(sd)
    del short[seed_util.SRC + "layers.1.fc2.bias"]
    with pytest.raises(KeyError, match="missing"):
        SEEDEncoderDot_NLL_LN(Config()).load_reference_state_dict(short)
    with pytest.raises(KeyError, match="unexpected"):
        SEEDEncoderDot_NLL_LN(Config()).load_reference_state_dict(dict(sd, **{"roberta.pooler.dense.weight": torch.zeros(1)}))
    with pytest.raises(KeyError):
        SEEDEncoderDot_NLL_LN.from_state_dict({k: v for k, v in sd.items() if ".layers." not in k})


def test_round_trip_into_the_encoders_names():
    """ance_amd.encoder.seed_state_dict(model.reference_state_dict()) with no renaming: the tensors the model holds, under the names
    Encoder reads for ARCH_SEED."""
    from ance_amd import encoder
    from ance_amd.model import SEEDEncoderDot_NLL_LN
    sd = _sd()
    m = SEEDEncoderDot_NLL_LN.from_state_dict(sd)
    got, want = encoder.seed_state_dict(m.reference_state_dict()), encoder.seed_state_dict(sd)
    assert sorted(got) == sorted(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_towers_refuse_each_others_batches():
    """A PackedTokens carries the rule it was made under: "seed" only from pack_tokens_by_id, so a RoBERTa tower refuses a SEED
    batch and the SEED tower a RoBERTa one, on the host."""
    from ance_amd.model import RobertaDot_NLL_LN, SEEDEncoderDot_NLL_LN, TowerConfig
    from ance_amd.packing import PackedTokens, PackRule
    z = torch.zeros(4, dtype=torch.int32)

    def batch(mode):
        return PackedTokens(z, None, z, torch.zeros(2, dtype=torch.int32), z[:1], 4, 4, torch.zeros((), dtype=torch.int64),
                            PackRule.of(mode, 1, VOCAB, MAX_POS))

    seed = SEEDEncoderDot_NLL_LN(Config(encoder_layers=1))
    rob = RobertaDot_NLL_LN(TowerConfig(VOCAB, 768, 1, 3072, MAX_POS, 1, 1e-5, 1))
    with pytest.raises(_lib.AnceLibraryError, match="made under"):
        seed.body_emb(batch("roberta"))
    with pytest.raises(_lib.AnceLibraryError, match="made under"):
        rob.body_emb(batch("seed"))
    assert seed.packed_dropped is None and rob.packed_dropped is None   # refused before the counter moves
