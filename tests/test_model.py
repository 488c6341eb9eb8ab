"""CPU checks of what the GPU tests of the first-row attention core and of ance_amd/model.py stand on (tests/model_util.py), and of
the models' plumbing that needs no GPU: names, checkpoint round trip, the MaxP reshaping."""
import numpy as np
import pytest
import torch

import attention_train_util as A
import layer_tail_util as T
import model_util as M
import train_step_util as S

SEED = 0x5EED0123456789AB


# ------------------------------------------------------------------------------------------------------------------ the kernel's statement
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_restated_gradient_against_autograd_fp64(p):
    lens, nh, L = (7, 0, 1, 33), 12, 33
    q0, k, v, g, ln = M.first_row_inputs("cpu", lens, nh, L)
    keep = M.first_row_keep(p, SEED, 3, ln, nh, L) if p > 0 else None
    want = M.autograd_first_row(q0, k, v, g, ln, nh, keep, p)
    got = M.first_row_fp64(q0, k, v, g, ln, nh, keep, p)
    for n in M.NAMES:
        assert np.abs(got[n] - want[n]).max() <= 1e-13 * max(1.0, np.abs(want[n]).max()), n
        assert np.abs(want[n]).max() > 0, n
    assert np.all(got["dk"][0, 7:] == 0) and np.all(got["dk"][1] == 0) and np.all(got["ctx"][1] == 0)


def test_first_row_is_row_zero_of_the_full_statement():
    """The statement equals query row 0 of attention_train_util.attention_fp64 with the full core's mask, dctx nonzero in row 0 only:
    the first-row mask IS the full mask's query row 0."""
    lens, nh, L, p = (9, 33, 2), 12, 33, 0.5
    q0, k, v, g, ln = M.first_row_inputs("cpu.full", lens, nh, L)
    keep_full = A.keep_masks(p, SEED, 5, ln, nh, L)
    keep = M.first_row_keep(p, SEED, 5, ln, nh, L)
    assert np.array_equal(keep, keep_full[:, :, 0])
    assert 0.3 < keep.mean() < 0.7
    q = A.seeded_inputs("cpu.full.q", lens, nh, L=L)[0]
    q[:, 0] = q0
    dctx = np.zeros_like(q)
    dctx[:, 0] = g
    full = A.attention_fp64(q, k, v, dctx, ln, nh, keep_full, p)
    got = M.first_row_fp64(q0, k, v, g, ln, nh, keep, p)
    for n, w in (("ctx", full["ctx"][:, 0]), ("dq", full["dq"][:, 0]), ("dk", full["dk"]), ("dv", full["dv"])):
        assert np.abs(got[n] - w).max() <= 1e-12, n
    assert np.all(full["dq"][:, 1:] == 0)


@pytest.mark.parametrize("dt", [None, torch.float16, torch.bfloat16])
def test_eager_expression_is_near_fp64(dt):
    """The reference of the bounds is sane: fp32 eager within 1e-5, the autocast expression within a few ulp of its dtype."""
    (q0, k, v, g, ln), want, ref, _ = M.reference("cpu.eager", (5, 64, 0, 130), 12, 130, 1.0, 0.1, SEED, 0, dt)
    tol = 1e-5 if dt is None else (2e-2 if dt == torch.float16 else 1e-1)
    for n in M.NAMES:
        assert 0 < ref[n] < tol, (n, ref[n])


# ------------------------------------------------------------------------------------------------------------------ the model's masks
def test_full_size_masks_carry_the_b_row_masks_at_the_first_rows():
    cfg, p, lens, L, off = S.BASE, 0.1, (12, 5, 1), 12, 14
    full = S.step_masks(p, SEED, off, cfg, lens, L)
    mine = M.first_row_masks(p, SEED, off, cfg, lens, L)
    B, H = len(lens), cfg["H"]
    assert np.array_equal(full["embeddings"], mine["embeddings"])
    for a, b in zip(full["layers"][0], mine["layers"][0]):
        assert np.array_equal(a, b)
    last = off + 1 + 3 * (cfg["N"] - 1)
    att, t1, t2 = mine["layers"][-1]
    assert np.array_equal(att[:, :, 0], M.first_row_keep(p, SEED, last, lens, cfg["heads"], L))
    for k, t in ((1, t1), (2, t2)):
        assert t.shape == (B * L, H)
        assert np.array_equal(t[np.arange(B) * L], T.tail_keep_mask(p, SEED, last + k, B, H))
        assert not np.array_equal(t[np.arange(B) * L], full["layers"][-1][k][np.arange(B) * L])   # row b of B rows is not row b * L


def test_the_models_oracle_is_the_towers():
    """model_util.tower_forward with a head of width H is train_step_util.tower_forward, bit for bit."""
    cfg = dict(S.BASE, N=1)
    sd = S.tower_state(cfg)
    call = S.batches(cfg)[0]
    masks = M.first_row_masks(0.1, SEED, 0, cfg, call["lens"], call["ids"].shape[1])
    W = {k: torch.from_numpy(v) for k, v in sd.items()}
    want = S.tower_forward(W, call, cfg, masks, 0.1)
    got = M.tower_forward(W, call, cfg, masks, 0.1, prefix="")
    assert torch.equal(want, got)


# ------------------------------------------------------------------------------------------------------------------ names, checkpoints
def _small_state(prefixes, head, cfg=S.LARGE):
    sd = {}
    for pre in prefixes:
        sd.update({k: v for k, v in M.model_state(cfg, prefix=pre).items() if k.startswith(pre) or head})
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


def test_state_dict_names_are_the_encoders():
    from ance_amd import model
    from ance_amd.encoder import weight_names
    sd = _small_state(("roberta.",), True)
    for cls in (model.RobertaDot_NLL_LN, model.RobertaDot_CLF_ANN_NLL_MultiChunk):
        m = cls.from_state_dict(sd)
        assert list(m.state_dict().keys()) == weight_names("roberta.", 1, True)
        assert [n for n, _ in m.named_parameters()] == weight_names("roberta.", 1, True)
        assert tuple(m.embeddingHead.weight.shape) == (768, 1024) and m.norm.eps == 1e-5
        assert m.roberta.embeddings.position_mode == "roberta" and m.roberta.embeddings.pad_token_id == 1
    cfg = dict(S.BASE, eps=1e-12)
    sd2 = _small_state(("question_model.", "ctx_model."), False, cfg)
    b = model.BiEncoder.from_state_dict(sd2, dropout=0.0)
    assert list(b.state_dict().keys()) == weight_names("question_model.", 2, False) + weight_names("ctx_model.", 2, False)
    e = b.ctx_model.embeddings
    assert e.position_mode == "absolute" and e.layer_norm_eps == 1e-12 and e.token_type_embeddings.weight.shape[0] == 2
    assert b.ctx_model.encoder.layer[1].hidden_dropout_prob == 0.0


def test_checkpoint_round_trip_and_refused_keys():
    from ance_amd import model
    sd = _small_state(("roberta.",), True)
    extras = {"roberta.pooler.dense.weight": torch.randn(4, 4), "roberta.pooler.dense.bias": torch.randn(4),
              "classifier.dense.weight": torch.randn(3, 3), "classifier.out_proj.bias": torch.randn(2),
              "roberta.embeddings.position_ids": torch.arange(514)[None]}
    full = dict(sd, **extras)
    m = model.RobertaDot_NLL_LN.from_state_dict(full)
    assert not any(k in m.state_dict() for k in extras)
    out = m.reference_state_dict()
    assert sorted(out) == sorted(full)
    for k, v in full.items():
        assert torch.equal(out[k], v), k
    with pytest.raises(KeyError, match="unexpected"):
        m.load_reference_state_dict(dict(full, **{"roberta.encoder.layer.0.attention.self.query.scale": torch.zeros(1)}))
    with pytest.raises(KeyError, match="missing"):
        m.load_reference_state_dict({k: v for k, v in full.items() if k != "norm.bias"})
    b = model.BiEncoder.from_state_dict(dict(_small_state(("question_model.", "ctx_model."), False, S.BASE),
                                             **{"ctx_model.pooler.dense.weight": torch.zeros(2, 2)}))
    assert "ctx_model.pooler.dense.weight" in b.reference_state_dict()
    with pytest.raises(KeyError, match="unexpected"):
        b.load_reference_state_dict(dict(b.reference_state_dict(), **{"encode_proj.weight": torch.zeros(1)}))


def test_use_mean_is_refused():
    from ance_amd import _lib, model

    class Arg:
        use_mean = True

    cfg = model.TowerConfig(100, 768, 1, 3072, 514, 1, 1e-5, 1)
    with pytest.raises(_lib.AnceLibraryError, match="use_mean"):
        model.RobertaDot_NLL_LN(cfg, Arg())
    Arg.use_mean = False
    assert model.RobertaDot_NLL_LN(cfg, Arg()).use_mean is False


# ------------------------------------------------------------------------------------------------------------------ MaxP
def test_maxp_reshaping_and_the_mask_column():
    """body_emb's reshaping and forward's mask column against the reference's expressions (model/models.py:103-109, 165-199)."""
    from ance_amd import model
    B, C, base = 3, 2, 512
    ids = torch.arange(B * C * base).reshape(B, C * base)
    lens = torch.tensor([700, 512, 3])
    mask = (torch.arange(C * base)[None, :] < lens[:, None]).long()
    got = model.RobertaDot_CLF_ANN_NLL_MultiChunk.chunk_mask(mask, C)
    want = mask.reshape(B, C, -1)[:, :, 0]
    assert got.dtype == torch.float32 and torch.equal(got, want.float())
    assert got.tolist() == [[1.0, 1.0], [1.0, 0.0], [1.0, 0.0]]
    # the reference's inverted bias from it
    assert torch.equal(((1 - got) * (-9999)).float(), ((1 - want) * (-9999)).float())

    seen = {}

    class Probe(model.RobertaDot_CLF_ANN_NLL_MultiChunk):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.base_len = 512
            self.roberta = lambda i, m: seen.update(ids=i, mask=m) or torch.zeros(i.shape[0], 4)
            self._head = lambda rows: torch.arange(rows.shape[0] * 768, dtype=torch.float32).reshape(rows.shape[0], 768)

    out = Probe().body_emb(ids, mask)
    full_length = C * base
    want_ids = ids.reshape(B, C, full_length // C).reshape(B * C, full_length // C)
    assert torch.equal(seen["ids"], want_ids) and torch.equal(seen["mask"], mask.reshape(B * C, base))
    assert tuple(out.shape) == (B, C, 768) and torch.equal(out, torch.arange(B * C * 768, dtype=torch.float32).reshape(B, C, 768))
    assert (seen["mask"].sum(1) == torch.tensor([512, 188, 512, 0, 3, 0])).all()   # all-pad chunks have length 0
