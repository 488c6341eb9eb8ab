"""The trained-like golden vectors (tests/golden/make_golden_trained.py: the reference's own RobertaDot_NLL_LN / HFBertEncoder at
12 layers on oracle.encoder_ref.trained_like_state_dict weights) on the CPU: the weights reproduce their checksum, the oracle's fp32
restatement reproduces the committed outputs, and the reference's own fp32-vs-fp64 distance -- the yardstick of the GPU tests'
bound, max(2e-5, 4 x it) -- is small enough for that bound to pin something."""
import json
import os

import numpy as np
import pytest
import torch

from golden_util import golden_weights
from oracle import encoder_ref

torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))

BERT = dict(kind="bert", vocab=30522, max_pos=512, head=False, prefixes=("ctx_model.",))
FIXTURES = {"firstp12_trained": {}, "firstp12_trained_L512": {}, "bert12_trained": BERT}


@pytest.fixture(scope="module")
def manifest(golden_dir):
    with open(os.path.join(golden_dir, "trained_manifest.json")) as f:
        return json.load(f)["encoder"]


_weights = {}


def weights(meta, kw):
    """One build per weight set (the two FirstP fixtures share theirs); golden_weights fails on a checksum mismatch."""
    if meta["checksum"] not in _weights:
        _weights.clear()
        _weights[meta["checksum"]] = golden_weights(meta, **kw)
    return _weights[meta["checksum"]]


@pytest.mark.parametrize("fixture", list(FIXTURES))
def test_trained_like_golden_matches_reference(golden_dir, manifest, fixture):
    meta = manifest[fixture]
    assert meta["gen"] == "det" and meta["n_layers"] == 12
    sd = weights(meta, FIXTURES[fixture])
    assert encoder_ref.state_dict_sha256(sd) == meta["checksum"]
    g = np.load(os.path.join(golden_dir, "encoder_%s.npz" % fixture))
    assert sorted(g.files) == ["emb", "ids", "lens"]
    ids = torch.from_numpy(g["ids"])
    with torch.no_grad():
        if fixture.startswith("bert"):
            emb = encoder_ref.bert_cls(sd, ids, (ids != 0).long(), "ctx_model.", n_layers=12)
        else:
            emb = encoder_ref.rdot_nll_ln_emb(sd, ids, encoder_ref.mask_from_lengths(g["lens"], ids.shape[1]), n_layers=12)
    assert emb.dtype == torch.float32 and g["emb"].dtype == np.float32
    d = float(np.abs(emb.numpy().astype(np.float64) - g["emb"]).max())
    print("%s: oracle fp32 vs golden %.3e, reference fp32 vs fp64 %.3e" % (fixture, d, meta["fp32_vs_fp64"]))
    assert d <= 1e-6, d
    # a condition on the fixture, not a measurement of any code under test: above it, 4 x the distance admits errors above 1e-3
    assert np.isfinite(meta["fp32_vs_fp64"]) and 0.0 < meta["fp32_vs_fp64"] < 2.5e-4, meta["fp32_vs_fp64"]


def test_trained_like_fixtures_hold_the_stated_cases(golden_dir, manifest):
    """The lengths and the interior pad ids the fixtures exist for."""
    g = np.load(os.path.join(golden_dir, "encoder_firstp12_trained.npz"))
    assert g["ids"].shape == (13, 128) and g["lens"].tolist()[:11] == [1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128]
    inside = [int(((g["ids"][r] == 1) & (np.arange(128) < g["lens"][r])).sum()) for r in range(13)]
    assert inside == [0] * 11 + [1, 3]
    g5 = np.load(os.path.join(golden_dir, "encoder_firstp12_trained_L512.npz"))
    assert g5["ids"].shape == (6, 512) and g5["lens"].tolist() == [1, 255, 256, 257, 511, 512]
    gb = np.load(os.path.join(golden_dir, "encoder_bert12_trained.npz"))
    assert gb["ids"].shape == (7, 256) and gb["lens"].tolist() == [1, 3, 64, 128, 129, 255, 256]
    assert manifest["firstp12_trained"]["checksum"] == manifest["firstp12_trained_L512"]["checksum"]
    assert manifest["firstp12_trained"]["trained"]["ffn_drive"] == 300.0
    # unit-variance rows behind the head's LayerNorm; the raw [CLS] rows of the BERT tower carry the outlier gains
    assert 0.9 < float(g["emb"].std()) < 1.1 and float(np.abs(gb["emb"]).max()) > 100.0


def test_trained_like_generator_keeps_the_construction():
    """The edits of trained_like_state_dict, on a 2-layer tower, against the plain deterministic weights of the same seed."""
    kw = dict(n_layers=2, seed=7, ln_jitter=0.1, vocab=64, max_pos=16)
    base = encoder_ref.det_state_dict(**kw)
    sd = encoder_ref.trained_like_state_dict(2, ffn_drive=300.0, seed=7, vocab=64, max_pos=16)
    assert sorted(sd) == sorted(base)
    changed = {k for k in sd if not torch.equal(sd[k], base[k])}
    ln = ["roberta.embeddings.LayerNorm.weight"] + ["roberta.encoder.layer.%d.%sLayerNorm.weight" % (i, p) for i in range(2)
                                                      for p in ("attention.output.", "output.")]
    qk = ["roberta.encoder.layer.%d.attention.self.%s.weight" % (i, n) for i in range(2) for n in ("query", "key")]
    assert changed == set(ln + qk + ["roberta.embeddings.word_embeddings.weight", "roberta.encoder.layer.1.intermediate.dense.bias"])
    for k in ln:
        assert sd[k][17] == base[k][17] * 50.0 and sd[k][400] == base[k][400] * -50.0
        rest = [i for i in range(768) if i not in (17, 400)]
        assert torch.equal(sd[k][rest], base[k][rest])
    for k in qk:
        assert torch.equal(sd[k], base[k] * 6.0)
    we, we0 = sd["roberta.embeddings.word_embeddings.weight"], base["roberta.embeddings.word_embeddings.weight"]
    assert torch.equal(we[:, 6:], we0[:, 6:] * 1.4) and torch.allclose(we[:, 5], we0[:, 5] * 1.4 + 0.04, rtol=0, atol=1e-7)
    b = sd["roberta.encoder.layer.1.intermediate.dense.bias"]
    assert b[123] == 300.0 and torch.equal(b[:123], base["roberta.encoder.layer.1.intermediate.dense.bias"][:123])
    assert torch.equal(sd["norm.weight"], base["norm.weight"])   # the head's LayerNorm is left alone
