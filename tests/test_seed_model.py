"""SEED-Encoder (model_type seeddot_nll) on the host: the checkpoint-name mapping onto the encoder's weight order, the checks
of load_model, and the tokenizer refusal.  No GPU."""
import json
import os
import types

import pytest
import torch

from seed_util import SRC, to_seed_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hf_state_dict(n_layers=2, H=16, inter=32, vocab=40, max_pos=20):
    g = torch.Generator().manual_seed(0)
    sd = {}
    e = "roberta.embeddings."
    for k, shape in ((e + "word_embeddings.weight", (vocab, H)), (e + "position_embeddings.weight", (max_pos, H)),
                     (e + "token_type_embeddings.weight", (1, H)), (e + "LayerNorm.weight", (H,)), (e + "LayerNorm.bias", (H,))):
        sd[k] = torch.randn(*shape, generator=g)
    for i in range(n_layers):
        p = "roberta.encoder.layer.%d." % i
        for k, o, n in (("attention.self.query", H, H), ("attention.self.key", H, H), ("attention.self.value", H, H),
                        ("attention.output.dense", H, H), ("intermediate.dense", inter, H), ("output.dense", H, inter)):
            sd[p + k + ".weight"] = torch.randn(o, n, generator=g)
            sd[p + k + ".bias"] = torch.randn(o, generator=g)
        for k in ("attention.output.LayerNorm", "output.LayerNorm"):
            sd[p + k + ".weight"] = torch.randn(H, generator=g)
            sd[p + k + ".bias"] = torch.randn(H, generator=g)
    sd["embeddingHead.weight"] = torch.randn(768, H, generator=g)
    sd["embeddingHead.bias"] = torch.randn(768, generator=g)
    sd["norm.weight"] = torch.randn(768, generator=g)
    sd["norm.bias"] = torch.randn(768, generator=g)
    return sd


def _seed_checkpoint_dict(hf):
    sd = to_seed_names(hf)
    # what a SEED checkpoint carries besides the encoder: must be ignored
    sd["classification_heads.dense.weight"] = torch.ones(16, 16)
    sd["classification_heads.out_proj.bias"] = torch.ones(2)
    sd["decoder.layers.0.fc1.weight"] = torch.ones(8, 8)
    sd["decoder.embed_tokens.weight"] = torch.ones(40, 8)
    return sd


def test_arch_seed_is_two_in_the_header_and_the_binding():
    from ance_amd.encoder import ARCH_BERT, ARCH_ROBERTA, ARCH_SEED
    assert (ARCH_ROBERTA, ARCH_BERT, ARCH_SEED) == (0, 1, 2)
    with open(os.path.join(ROOT, "include", "ance_amd.h")) as f:
        assert "#define ANCE_ARCH_SEED 2" in f.read()


def test_seed_state_dict_maps_every_weight_in_the_encoder_order():
    from ance_amd.encoder import count_layers, seed_state_dict, weight_names
    hf = _hf_state_dict()
    sd = _seed_checkpoint_dict(hf)
    m = seed_state_dict(sd)
    assert count_layers(m, "seed.") == 2
    names = weight_names("seed.", 2, True)
    assert sorted(m) == sorted(names)  # nothing from classification_heads.* / decoder.*
    for k in names:
        hk = k.replace("seed.", "roberta.", 1)
        if k.endswith("token_type_embeddings.weight"):
            assert tuple(m[k].shape) == (1, 16) and not m[k].any()  # no segment embedding: a zero row adds nothing
        else:
            assert m[k] is hf[hk], k  # the tensors themselves, not copies
    assert sd[SRC + "layers.1.self_attn.q_proj.weight"] is m["seed.encoder.layer.1.attention.self.query.weight"]
    assert sd[SRC + "layers.0.fc2.weight"] is m["seed.encoder.layer.0.output.dense.weight"]
    assert sd[SRC + "layers.0.final_layer_norm.bias"] is m["seed.encoder.layer.0.output.LayerNorm.bias"]


def test_seed_state_dict_rejects_missing_and_misshapen_weights():
    from ance_amd.encoder import seed_state_dict
    hf = _hf_state_dict()
    sd = _seed_checkpoint_dict(hf)
    with pytest.raises(KeyError):
        seed_state_dict({k: v for k, v in sd.items() if not k.endswith("layers.1.self_attn.v_proj.bias")})
    with pytest.raises(KeyError):
        seed_state_dict({k: v for k, v in sd.items() if not k.startswith("norm.")})
    with pytest.raises(KeyError):
        seed_state_dict(hf)  # HF RoBERTa names are not a SEED checkpoint
    bad = dict(sd)
    bad[SRC + "layers.0.fc1.weight"] = torch.zeros(32, 15)
    with pytest.raises(ValueError, match="fc1|intermediate"):
        seed_state_dict(bad)
    bad = dict(sd)
    bad["embeddingHead.weight"] = torch.zeros(200, 16)
    with pytest.raises(ValueError, match="embeddingHead"):
        seed_state_dict(bad)


def test_load_model_checks_config_json_against_the_checkpoint(tmp_path):
    from ance_amd.encoder import load_model
    torch.save(_seed_checkpoint_dict(_hf_state_dict(max_pos=514)), str(tmp_path / "pytorch_model.bin"))
    (tmp_path / "config.json").write_text(json.dumps({"encoder_layers": 12, "pad_token_id": 1, "max_positions": 512}))
    with pytest.raises(ValueError, match="encoder_layers=12"):
        load_model("seeddot_nll", str(tmp_path))
    (tmp_path / "config.json").write_text(json.dumps({"encoder_layers": 2, "pad_token_id": 1, "max_positions": 256}))
    with pytest.raises(ValueError, match="max_positions=256"):
        load_model("seeddot_nll", str(tmp_path))


def test_load_tokenizer_refuses_seed_and_names_the_reference_preprocess():
    from ance_amd.msmarco_data import load_tokenizer
    args = types.SimpleNamespace(model_type="seeddot_nll", model_name_or_path="unused")
    with pytest.raises(ValueError, match="reference's preprocess"):
        load_tokenizer(args)
