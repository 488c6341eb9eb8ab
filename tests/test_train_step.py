"""The oracle of tests/test_gpu_train_step.py checked against itself on the CPU (tests/train_step_util.py): the torch float64 tower
is held to the hand-written NumPy fp64 restatements of its pieces, to the NumPy objectives and to finite differences of its own
loss, and step_masks to the per-piece mask functions -- so that the GPU test's reference is not one implementation's word."""
import functools

import numpy as np
import pytest
import torch

import attention_train_util as A
import embeddings_util as E
import layer_tail_util as T
import objective_util as O
import train_step_util as S

SEED = S.SEED
REL = 1e-11


def _close(tag, got, want, scale=None):
    d = float(np.abs(np.asarray(got, np.float64) - want).max())
    s = float(np.abs(want).max()) if scale is None else scale
    print("%-60s max|delta| %.3e  scale %.3e  relative %.3e" % (tag, d, s, d / s))
    assert d <= REL * s, (tag, d, s)


@functools.lru_cache(maxsize=None)
def _step0(kind):
    """The first step's calls, masks (p 0.1) and fp64 result."""
    cfg = S.BASE if kind == "triplet" else S.LARGE
    sd = S.tower_state(cfg)
    calls = S.step_calls(cfg, kind, 0)
    masks = S.calls_masks(0.1, SEED, 0, cfg, calls)
    return cfg, sd, calls, masks, S.tower_fp64(sd, calls, cfg, kind, masks, 0.1)


def test_one_layer_of_the_tower_is_layer_fp64():
    """(a) layer_torch_forward in float64 -- the tower's layer -- against layer_tail_util.layer_fp64 (NumPy, hand-written backward)
    with the three masks: the output, the input gradient and every parameter gradient to 1e-11 relative.  attention.self.key.bias
    has no gradient (both sides hold fp64 rounding noise, 1e-17): it is held to 1e-11 of query.bias's scale."""
    H, heads, inter, eps, p, lens, L = 768, 12, 3072, 1e-5, 0.1, np.asarray((4, 7, 9), np.int32), 9
    B = len(lens)
    sd = T.layer_weights(H, inter)
    hs, dout = T.det_normal(3, "train.hs", (B, L, H), 1.0), T.det_normal(3, "train.dout", (B, L, H), 0.1)
    keeps = (A.keep_masks(p, SEED, 0, lens, heads, L), T.tail_keep_mask(p, SEED, 1, B * L, H), T.tail_keep_mask(p, SEED, 2, B * L, H))
    want = T.layer_fp64(hs, lens, sd, heads, eps, dout, keeps, p, p)
    rows = torch.from_numpy(A._valid(lens, L))
    W = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in sd.items()}
    ths = torch.from_numpy(hs).double().requires_grad_(True)
    out = T.layer_torch_forward(ths, rows, W, heads, eps, tuple(torch.from_numpy(m).double() for m in keeps), p, p)
    out.backward(torch.from_numpy(dout).double() * rows[:, :, None])
    valid = rows[:, :, None].numpy()
    _close("out", np.where(valid, out.detach().numpy(), 0), np.where(valid, want["out"], 0))
    _close("dhs", np.where(valid, ths.grad.numpy(), 0), np.where(valid, want["dhs"], 0))
    for n in T.LAYER_PARAMS:
        scale = np.abs(want["attention.self.query.bias"]).max() if n == "attention.self.key.bias" else None
        _close(n, W[n].grad.numpy(), want[n], scale)


@pytest.mark.parametrize("mode,pad,n_types", [("absolute", 0, 2), ("roberta", 1, 1)])
def test_the_embeddings_of_the_tower_are_embed_fp64(mode, pad, n_types):
    """(b) embed_torch_forward in float64 against embeddings_util.embed_fp64 on a step's own query and negative batches."""
    cfg = dict(S.BASE, mode=mode, pad=pad, n_types=n_types)
    tables = E.embed_inputs("tower", cfg["H"], S.VOCAB, S.MAX_POS, n_types, 73)
    for call in (S.batches(cfg)[0], S.batches(cfg)[2]):
        n = call["ids"].size
        keep, dy = E.tail_keep_mask(0.1, SEED, 5, n, cfg["H"]), E.embed_dy("train", n, cfg["H"])
        want = E.embed_fp64(call["ids"], call["types"], *tables, cfg["eps"], dy, mode, pad, keep, 0.1)
        W = [torch.from_numpy(t).double().requires_grad_(True) for t in tables]
        y = E.embed_torch_forward(call["ids"], call["types"], *W, cfg["eps"], mode, pad, torch.from_numpy(keep).double(), 0.1)
        y.backward(torch.from_numpy(dy).double().view(y.shape))
        _close(mode + " y", y.detach().numpy().reshape(n, -1), want["y"])
        assert pad in want["word_rows"] and not want["dword"][want["word_rows"] == pad].any()
        _close(mode + " dword", W[0].grad.numpy()[want["word_rows"]], want["dword"])
        rest = np.setdiff1d(np.arange(S.VOCAB), want["word_rows"])
        assert not W[0].grad.numpy()[rest].any()
        for g, k in zip(W[1:], ("dpos", "dtype", "dgamma", "dbeta")):
            _close("%s %s" % (mode, k), g.grad.numpy(), want[k])


@pytest.mark.parametrize("kind", ["triplet", "inbatch"])
def test_the_loss_is_the_numpy_objective_and_every_sequence_carries_gradient(kind):
    """The torch loss and its gradients into the three embeddings against objective_util's fp64 objectives, and the premise of the
    batches' seeds: every triplet's negative leads (every query's positive trails), so no sequence's gradient is a rounded zero."""
    cfg, sd, calls, masks, r = _step0(kind)
    embs = [torch.from_numpy(e).requires_grad_(True) for e in r["embs"]]
    loss = S.loss_torch(kind, embs)
    loss.backward()
    if kind == "triplet":
        want = O.nll_fp64(*r["embs"])
        grads = (want["gq"], want["ga"], want["gb"])
        lead = want["logits"][:, 1] - want["logits"][:, 0]
    else:
        want = O.inbatch_fp64(r["embs"][0], r["embs"][1], np.arange(3))
        grads = (want["gq"], want["gctx"])
        s = want["scores"]
        lead = np.array([np.delete(s[i], i).max() - s[i, i] for i in range(3)])
    print(kind, "loss", r["loss"], "leads", lead)
    assert abs(float(loss.detach()) - want["loss"]) <= REL * abs(want["loss"]) and abs(r["loss"] - want["loss"]) <= REL * abs(want["loss"])
    for e, g in zip(embs, grads):
        _close(kind + " embedding gradient", e.grad.numpy(), g)
    assert np.all(lead > 5.0), lead


# (name, flat indices): a word row that occurs in all three calls (777 is a first token, 77 occurs twice in a sequence), a position
# row, both LayerNorms of layer 0, query.weight, output.dense.bias and the head
FD_COORDS = (("embeddings.word_embeddings.weight", (777 * 768 + 6, 777 * 768 + 400, 77 * 768 + 123)),
             ("embeddings.position_embeddings.weight", (2 * 768 + 9, 0 * 768 + 700)),
             ("encoder.layer.0.attention.output.LayerNorm.weight", (3, 511)), ("encoder.layer.0.attention.output.LayerNorm.bias", (64, 767)),
             ("encoder.layer.0.output.LayerNorm.weight", (100, 640)), ("encoder.layer.0.output.LayerNorm.bias", (0, 333)),
             ("encoder.layer.0.attention.self.query.weight", (7 * 768 + 11, 300 * 768 + 301, 767 * 768 + 2)),
             ("encoder.layer.1.output.dense.bias", (17, 600)),
             ("embeddingHead.weight", (10 * 768 + 20, 500 * 768 + 499)), ("norm.weight", (42,)), ("norm.bias", (700,)))


def test_central_differences_of_the_fp64_loss_agree_with_autograd():
    """(c) 22 coordinates, h = 1e-4: |(L(x + h) - L(x - h)) / 2h - autograd| <= 1e-6 of the autograd value, with the masks held.
    The difference quotient has a noise floor of its own: the loss is a mean of logits near 500, known to a few 2^-52 of that, so
    the quotient is known to about 1e-9 absolute -- the coordinates are ones whose gradient is above 1e-3 (measured: 1.2e-7 relative at
    the smallest of them, 4e-3; at most 3e-8 elsewhere)."""
    cfg, sd, calls, masks, r = _step0("triplet")
    W = {k: torch.from_numpy(v).double() for k, v in sd.items()}

    def loss():
        with torch.no_grad():
            return float(S.loss_torch("triplet", [S.tower_forward(W, c, cfg, m, 0.1) for c, m in zip(calls, masks)]))

    assert abs(loss() - r["loss"]) <= REL * r["loss"]
    h, bad = 1e-4, []
    for name, coords in FD_COORDS:
        flat = W[name].view(-1)
        for i in coords:
            x = float(flat[i])
            flat[i] = x + h
            up = loss()
            flat[i] = x - h
            down = loss()
            flat[i] = x
            fd, g = (up - down) / (2 * h), float(r["grads"][name].reshape(-1)[i])
            print("%-52s [%6d] autograd % .9e  central difference % .9e  relative %.2e" % (name, i, g, fd, abs(fd - g) / abs(g)))
            if not abs(fd - g) <= 1e-6 * abs(g):
                bad.append((name, i, g, fd))
    assert not bad, bad


def test_step_masks_are_the_pieces_masks_at_consecutive_offsets():
    """(d) step_masks at first_offset k: embeddings at k, then per layer the attention, the first tail, the second tail at k + 1,
    k + 2, ...; the calls of a step take consecutive blocks of 1 + 3 N."""
    cfg, p, k = S.BASE, 0.1, 21
    calls = S.batches(cfg)
    per_call = S.draws_per_call(cfg)
    assert per_call == 7
    got = S.calls_masks(p, SEED, k, cfg, calls)
    seen = []
    for c, m in zip(calls, got):
        B, L = c["ids"].shape
        assert np.array_equal(m["embeddings"], E.tail_keep_mask(p, SEED, k, B * L, cfg["H"]))
        seen.append(m["embeddings"])
        k += 1
        for ka, k1, k2 in m["layers"]:
            assert np.array_equal(ka, A.keep_masks(p, SEED, k, c["lens"], cfg["heads"], L))
            assert np.array_equal(k1, T.tail_keep_mask(p, SEED, k + 1, B * L, cfg["H"]))
            assert np.array_equal(k2, T.tail_keep_mask(p, SEED, k + 2, B * L, cfg["H"]))
            assert not np.array_equal(k1, k2)
            k += 3
    assert k == 21 + 3 * per_call
    assert not np.array_equal(seen[1], seen[2][:len(seen[1])])   # two calls of one step do not share a mask
    assert S.calls_masks(0.0, SEED, 0, cfg, calls) == [None] * 3


def test_the_batches_cross_the_kernels_granularities():
    for cfg, kind in ((S.BASE, "triplet"), (S.LARGE, "inbatch")):
        for step in range(3 if kind == "triplet" else 2):
            calls = S.step_calls(cfg, kind, step)
            rows = [c["ids"].size for c in calls]
            assert all(r % 16 for r in rows) and len(set(rows)) == len(rows), rows
            lens = np.concatenate([c["lens"] for c in calls])
            assert {1, 17, 33} <= set(lens.tolist())
            for c in calls:
                ids, valid = c["ids"], A._valid(c["lens"], c["ids"].shape[1])
                assert np.all(ids[~valid] == cfg["pad"]) and (~valid).any() and np.all(ids[valid] != cfg["pad"])
                assert set(S.PLANTED) <= set(ids[valid].tolist()) and (ids[0] == S.PLANTED[1]).sum() >= 2
                assert ids.min() >= 0 and ids.max() < S.VOCAB
