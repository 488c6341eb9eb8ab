"""Generates tests/golden/seed_step.npz + seed_step.json from the reference itself (build container only): one training step's
forward and backward of the reference's own SEEDEncoderDot_NLL_LN (2 layers, make_golden_seed.build_seed_model) in eval mode, run
once in fp32 and once after .double(), on tests/seed_util.det_seed_state_dict weights (recorded as seed + sha256, never stored).

The batch: B = 4 triplets, queries L = 16, passages L = 64, ids folded into SEED's vocabulary (seed_util.into_seed_vocab), pad ids
planted INSIDE the records of all three calls at a fraction of about 0.2 (seed_util.interior_pads), one passage that is [CLS]
followed by pads only, no record that begins with a pad.

Stored: the ids; the fp64 run's loss, and its embeddings rounded to fp32; of the fp64 gradient of every used parameter what
tests/model_util.golden_view keeps (the whole tensor up to 4,096 elements, otherwise a fixed sample; of embed_tokens only the rows
that occur); per tensor ref_err = max |fp32 run - fp64 run| over the whole tensor; the list of the used parameter names in the
reference's own order (``classification_heads.*`` gets no gradient and is left out).  Asserted: every triplet's negative has
softmax weight >= 0.05 -- otherwise the comparison would be of zeros; the weight seed and the seed of the ids are searched until it
holds.

    python tests/golden/make_golden_seed_step.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import model_util as M  # noqa: E402
from make_golden_model import negative_weights  # noqa: E402
from make_golden_seed import build_seed_model  # noqa: E402
from oracle import encoder_ref, synth  # noqa: E402
from seed_util import SRC, det_seed_state_dict, interior_pads, into_seed_vocab  # noqa: E402

T = lambda x: torch.from_numpy(np.asarray(x)).long()  # noqa: E731
B, LQ, LP, PAD_FRAC = 4, 16, 64, 0.2
TOKENS = SRC + "embed_tokens.weight"


def used(name):
    return not name.startswith("classification_heads.")


def batch(ids_seed):
    rng = np.random.default_rng(ids_seed)
    ql = synth.lognormal_lengths(rng, B, 9, 0.35, 5, LQ)
    al = synth.lognormal_lengths(rng, B, 40, 0.45, 8, LP)
    bl = synth.lognormal_lengths(rng, B, 40, 0.45, 8, LP)
    qi, ai, bi = (into_seed_vocab(synth.make_records(rng, B, L, n)) for L, n in ((LQ, ql), (LP, al), (LP, bl)))
    qi, ai, bi = (interior_pads(rng, x, n, PAD_FRAC) for x, n in ((qi, ql), (ai, al), (bi, bl)))
    ai[3, 1:] = synth.PAD   # [CLS] followed by pads only
    for x in (qi, ai, bi):
        assert (x[:, 0] != synth.PAD).all()   # no leading pad
        if not ((x == synth.PAD) & (np.cumsum(x[:, ::-1] != synth.PAD, 1)[:, ::-1] > 0)).any():   # a pad with a token behind it
            return None
    return qi, ai, bi


def inputs_of(qi, ai, bi):
    out = []
    for x in (qi, ai, bi):
        out += [T(x), (T(x) != synth.PAD).long()]
    return tuple(out)


def run(model, inputs, double):
    """(loss, [embeddings], {name: gradient}) of one forward + backward of the reference's own forward."""
    model = model.double() if double else model.float()
    model.eval()
    model.zero_grad()
    loss = model(*inputs)[0]
    loss.backward()
    with torch.no_grad():
        embs = [model.query_emb(inputs[0], inputs[1]), model.body_emb(inputs[2], inputs[3]), model.body_emb(inputs[4], inputs[5])]
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if used(n)}   # every used parameter HAS a gradient
    return loss.detach(), [e.detach() for e in embs], grads


def search():
    """The first (weight seed, ids seed) at which every triplet's negative keeps a softmax weight >= 0.05."""
    for wseed in range(61, 71):
        w = dict(seed=wseed, n_layers=2, ln_jitter=0.1)
        sd = det_seed_state_dict(**w)
        m = build_seed_model(2, sd)
        for ids_seed in range(505, 545):
            ids = batch(ids_seed)
            if ids is None:   # a call without an interior pad
                continue
            inp = inputs_of(*ids)
            with torch.no_grad():
                embs = [m.query_emb(inp[0], inp[1]), m.body_emb(inp[2], inp[3]), m.body_emb(inp[4], inp[5])]
            wts, _ = negative_weights(embs)
            print("weight seed", wseed, "ids seed", ids_seed, "negative weights", ["%.3f" % float(x) for x in wts])
            if float(wts.min()) >= 0.05:
                return w, sd, m, ids_seed, ids
    raise AssertionError("no seed keeps every negative's weight >= 0.05")


def main():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    w, sd, m, ids_seed, (qi, ai, bi) = search()
    inputs = inputs_of(qi, ai, bi)
    names = [n for n, _ in m.named_parameters() if used(n)]
    l32, e32, g32 = run(m, inputs, False)
    l64, e64, g64 = run(m, inputs, True)
    wts, _ = negative_weights(e64)
    assert float(wts.min()) >= 0.05, wts
    assert sorted(g64) == sorted(names)
    rows = np.unique(np.concatenate([x.reshape(-1) for x in (qi, ai, bi)])).astype(np.int32)
    arrays = {"q_ids": qi, "a_ids": ai, "b_ids": bi, "rows." + TOKENS: rows}
    ref_err = {"loss": float((l32.double() - l64).abs())}
    for i, nm in enumerate("qab"):
        arrays["emb." + nm] = e64[i].numpy().astype(np.float32)   # held to the 2e-5 of the other pins, not to ref_err
        ref_err["emb." + nm] = float((e32[i].double() - e64[i]).abs().max())
    for n in names:
        full32, full64 = g32[n].double().numpy(), g64[n].numpy()
        if n == TOKENS:
            assert not np.delete(full64, rows, axis=0).any()   # nothing outside the rows that occur
            full32, full64 = full32[rows], full64[rows]
        ref_err[n] = float(np.abs(full32 - full64).max())
        arrays["grad." + n] = M.golden_view(n, full64)
    meta = dict(weights=dict(gen="det_seed", checksum=encoder_ref.state_dict_sha256(sd), **w), ids_seed=ids_seed, pad_frac=PAD_FRAC,
                loss=float(l64), ref_err=ref_err, negative_weight=[float(x) for x in wts], params=names, whole=M.WHOLE, sample=M.SAMPLE,
                torch=torch.__version__)
    print("loss", float(l64), "negative weights %.3f .. %.3f" % (float(wts.min()), float(wts.max())))
    np.savez_compressed(os.path.join(HERE, "seed_step.npz"), **arrays)
    with open(os.path.join(HERE, "seed_step.json"), "w") as f:
        json.dump(meta, f, indent=1)
    size = os.path.getsize(os.path.join(HERE, "seed_step.npz"))
    assert size <= os.path.getsize(os.path.join(HERE, "model_step.npz")), size
    print("seed_step.npz", size, "bytes")


if __name__ == "__main__":
    main()
