"""Large-tower shapes (RoBERTa-large width: hidden 1024, 16 heads) on the CPU: the descriptor rule of include/ance_amd.h, the byte
counts of the base tower (unchanged), and the config.json checks of ``load_model`` for rdot_nll / rdot_nll_multi_chunk."""
import ctypes
import json

import pytest
import torch

from ance_amd import _lib
from ance_amd.encoder import ARCH_BERT, ARCH_ROBERTA, ARCH_SEED, Encoder, check_roberta_config, load_model, weight_names

PRECISIONS = {"split": 1, "fp16": 2, "fp32": 3}


def desc(hidden=1024, n_heads=16, intermediate=4096, arch=ARCH_ROBERTA, has_head=1, precision=1, n_layers=24, max_tokens=32768):
    return _lib.AnceEncoderDesc(arch=arch, n_layers=n_layers, hidden=hidden, n_heads=n_heads, intermediate=intermediate,
                                vocab_size=50265, max_position=514, pad_token_id=1, ln_eps=1e-5, has_head=has_head, max_seq_len=512,
                                max_tokens=max_tokens, precision=precision)


def sizes(d):
    L = _lib.lib()
    return L.ance_encoder_weight_bytes(ctypes.byref(d)), L.ance_encoder_workspace_bytes(ctypes.byref(d))


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
def test_large_shape_is_accepted_in_every_mode(precision):
    w, x = sizes(desc(precision=PRECISIONS[precision]))
    assert w > 0 and x > 0
    # the large tower is bigger than the base one in both buffers
    wb, xb = sizes(desc(768, 12, 3072, n_layers=12, precision=PRECISIONS[precision]))
    assert w > 2 * wb and x > xb


@pytest.mark.parametrize("hidden,n_heads,kw", [
    (1024, 8, {}),                     # head dimension 128
    (1024, 12, dict(intermediate=3072)),  # head dimension not an integer
    (768, 6, dict(intermediate=3072)),    # head dimension 128 at base width
    (512, 8, dict(intermediate=2048)),    # hidden not 768 / 1024
    (1280, 20, dict(intermediate=5120)),
    (1024, 16, dict(arch=ARCH_BERT)),     # DPR's BiEncoder is bert-base
    (1024, 16, dict(arch=ARCH_SEED)),     # SEED's config is base width
    (1024, 16, dict(has_head=0)),         # a head-less large tower would emit 1024-wide rows
    (1024, 16, dict(intermediate=4224)),  # FFN1's N must be whole 256-column tiles at 1024
])
def test_unsupported_shapes_are_refused(hidden, n_heads, kw):
    for p in PRECISIONS.values():
        assert sizes(desc(hidden, n_heads, precision=p, **kw)) == (0, 0)


# ance_encoder_weight_bytes / _workspace_bytes of the base tower (12 layers, 768 / 12 / 3072, max_tokens 32768) on the parent
# commit: the large shape adds instances and must not move a byte of the base layout
BASE_BYTES = {
    "split": (669_235_456, 2_961_114_112),
    "fp16": (328_977_664, 1_350_501_376),
    "fp32": (668_826_880, 3_363_767_296),
}


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
def test_base_tower_byte_counts_are_unchanged(precision):
    got = sizes(desc(768, 12, 3072, n_layers=12, precision=PRECISIONS[precision]))
    assert got == BASE_BYTES[precision]


def _tiny_sd(hidden, inter, n_layers, vocab=16, max_pos=8):
    sd = {}
    for k in weight_names("roberta.", n_layers, True):
        if "word_embeddings" in k:
            shape = (vocab, hidden)
        elif "position_embeddings" in k:
            shape = (max_pos, hidden)
        elif "token_type" in k:
            shape = (1, hidden)
        elif k.startswith("embeddingHead.weight"):
            shape = (768, hidden)
        elif k.startswith(("embeddingHead", "norm.")):
            shape = (768,)
        elif "intermediate.dense.weight" in k:
            shape = (inter, hidden)
        elif "intermediate.dense.bias" in k:
            shape = (inter,)
        elif "output.dense.weight" in k and "attention" not in k:
            shape = (hidden, inter)
        elif k.endswith(".weight") and "LayerNorm" not in k:
            shape = (hidden, hidden)
        else:
            shape = (hidden,)
        sd[k] = torch.zeros(shape)
    return sd


LARGE_CFG = {"hidden_size": 1024, "num_attention_heads": 16, "intermediate_size": 4096, "num_hidden_layers": 2}


def test_config_json_gives_the_head_count():
    sd = _tiny_sd(1024, 4096, 2)
    assert check_roberta_config(LARGE_CFG, sd) == 16
    assert check_roberta_config({}, sd) is None  # no config.json: today's behaviour (hidden // 64 heads)
    base = _tiny_sd(768, 3072, 2)
    assert check_roberta_config({"hidden_size": 768, "num_attention_heads": 12}, base) == 12


@pytest.mark.parametrize("field,value", [("hidden_size", 768), ("intermediate_size", 3072), ("num_hidden_layers", 24)])
def test_config_json_disagreeing_with_the_weights_is_refused_by_name(field, value):
    cfg = dict(LARGE_CFG, **{field: value})
    with pytest.raises(ValueError, match=field):
        check_roberta_config(cfg, _tiny_sd(1024, 4096, 2))


def test_config_json_with_an_unsupported_head_count_lists_the_supported_shapes():
    with pytest.raises(ValueError, match="1024 / 16 heads"):
        check_roberta_config(dict(LARGE_CFG, num_attention_heads=8), _tiny_sd(1024, 4096, 2))


@pytest.mark.parametrize("model_type", ["rdot_nll", "rdot_nll_multi_chunk"])
def test_load_model_checks_config_json_before_building_the_encoder(tmp_path, model_type):
    torch.save(_tiny_sd(1024, 4096, 2), str(tmp_path / "pytorch_model.bin"))
    (tmp_path / "config.json").write_text(json.dumps(dict(LARGE_CFG, num_hidden_layers=3)))
    with pytest.raises(ValueError, match="num_hidden_layers=3"):
        load_model(model_type, str(tmp_path), max_seq_length=2048 if model_type.endswith("chunk") else 128)


def test_unsupported_tower_is_refused_with_the_supported_shapes():
    # hidden 512 (8 heads of 64): the size queries say 0 before anything is allocated
    with pytest.raises(_lib.AnceLibraryError, match="supported: hidden 768 / 12 heads.*hidden 1024 / 16 heads"):
        Encoder(_tiny_sd(512, 2048, 1), precision="split")
    with pytest.raises(_lib.AnceLibraryError, match="hidden 1024, 16 heads"):
        Encoder(_tiny_sd(1024, 4096, 1), arch=ARCH_BERT, prefix="roberta.", has_head=True, precision="split")
