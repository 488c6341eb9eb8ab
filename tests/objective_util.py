"""The trainers' objectives and the clipped LAMB step restated in fp64 NumPy -- the oracle of tests/test_objective.py,
tests/test_gpu_objective.py and tests/test_gpu_lamb_clip.py -- and the fixtures those tests share with
tests/golden/make_golden_objective.py (inputs are regenerated from oracle.encoder_ref.det_normal, never stored).

  triplet NLL   model/models.py:77-81 (FirstP), :103-134 (MaxP), :268-271 (DPR triplet form)
  in-batch      drivers/run_ann_dpr.py:356-365
  clipping      torch.nn.utils.clip_grad_norm_ (2-norm) in front of utils/lamb.py Lamb.step
"""
import math

import numpy as np

import lamb_util as U
from oracle.encoder_ref import det_normal

# ---------------------------------------------------------------------------------------------------------------- fixtures
# Embedding scale: logits of a few units, so that sigmoid / softmax are neither saturated nor flat.
TRIPLET_STD = 0.05
FIRSTP_CASES = {"firstp_n1": 1, "firstp_n3": 3, "firstp_n64": 64}   # d = 768
DPR_TRIPLET_CASES = {"dpr_n3": 3}                                      # BiEncoder.forward's triplet branch, d = 768
MAXP_N, MAXP_CHUNKS, D = 8, 4, 768
# valid chunks per row of a / b (trailing chunks masked); row 2 of a and row 3 of b keep chunk 0 only
MAXP_LEN_A = [4, 3, 1, 2, 4, 4, 2, 3]
MAXP_LEN_B = [4, 2, 3, 1, 4, 3, 4, 2]
MAXP_DUP = {"a": (4, 1, 3), "b": (5, 0, 2)}  # (row, chunk, chunk): exact duplicate rows -> an exact tie
INBATCH_CASES = {"inbatch_nq1": 1, "inbatch_nq7": 7, "inbatch_nq128": 128}   # nc = 2 nq, positives at 2 i
INBATCH_D = 128
INBATCH_DUP_ROWS = (3, 5)   # rows (where nq > 5) whose positive column is duplicated at a HIGHER and at a LOWER column
CLIP_STEPS = 3
CLIP_RUNS = {"clip": 1.0, "noclip": 1000.0}   # the fixture's gradient norm is ~7.7: 1.0 clips at every step, 1000 never
SAMPLE_STRIDE = 13            # tensors above SAMPLE_MIN elements are recorded at every 13th flat element
SAMPLE_MIN = 30000


def recorded(x):
    x = np.asarray(x).reshape(-1)
    return (x[::SAMPLE_STRIDE] if x.size > SAMPLE_MIN else x).copy()


def triplet_inputs(case):
    """(q, a, b, mask_a, mask_b) fp32; masks None for FirstP."""
    if case == "maxp":
        n, C = MAXP_N, MAXP_CHUNKS
        q = det_normal(11, "obj.maxp.q", (n, D), TRIPLET_STD * 4)
        a = det_normal(11, "obj.maxp.a", (n, C, D), TRIPLET_STD * 4)
        b = det_normal(11, "obj.maxp.b", (n, C, D), TRIPLET_STD * 4)
        for t, (r, c0, c1) in ((a, MAXP_DUP["a"]), (b, MAXP_DUP["b"])):
            # the duplicated pair must be the winner: align it with q
            t[r, c0] = q[r] * 0.5 + t[r, c0] * 0.1
            t[r, c1] = t[r, c0]
        ma = (np.asarray(MAXP_LEN_A)[:, None] > np.arange(C)[None, :]).astype(np.float32)
        mb = (np.asarray(MAXP_LEN_B)[:, None] > np.arange(C)[None, :]).astype(np.float32)
        return q, a, b, ma, mb
    n = dict(FIRSTP_CASES, **DPR_TRIPLET_CASES)[case]
    return (det_normal(11, "obj.%s.q" % case, (n, D), TRIPLET_STD), det_normal(11, "obj.%s.a" % case, (n, D), TRIPLET_STD * 20),
            det_normal(11, "obj.%s.b" % case, (n, D), TRIPLET_STD * 20), None, None)


def seeded_triplets(n, chunks, d=D, seed=23):
    """Larger seeded inputs without a golden: (q, a, b, mask_a, mask_b)."""
    tag = "obj.seeded.%d.%d" % (n, chunks)
    q = det_normal(seed, tag + ".q", (n, d), 0.2)
    shape = (n, d) if chunks == 1 else (n, chunks, d)
    a, b = det_normal(seed, tag + ".a", shape, 0.2), det_normal(seed, tag + ".b", shape, 0.2)
    if chunks == 1:
        return q, a, b, None, None
    la = 1 + (np.arange(n) * 7) % chunks
    lb = 1 + (np.arange(n) * 5 + 2) % chunks
    return (q, a, b, (la[:, None] > np.arange(chunks)[None, :]).astype(np.float32),
            (lb[:, None] > np.arange(chunks)[None, :]).astype(np.float32))


def inbatch_inputs(nq, d=INBATCH_D, seed=31, plant=3.0):
    """(q, ctx, positive_idx): nc = 2 nq, positives at 2 i, each planted (ctx[2 i] += plant q[i] / |q[i]|) so that its score leads
    the runner-up by a wide margin; rows INBATCH_DUP_ROWS get an exact duplicate of the positive column -- row 3 at a higher column
    (the positive stays the lowest argmax: correct), row 5 at a lower one (the duplicate wins the tie: not correct)."""
    nc = 2 * nq
    q = det_normal(seed, "obj.inbatch.%d.%d.q" % (nq, d), (nq, d), 1.0 / math.sqrt(d) * 2)
    ctx = det_normal(seed, "obj.inbatch.%d.%d.c" % (nq, d), (nc, d), 1.0 / math.sqrt(d) * 2)
    pos = np.arange(nq, dtype=np.int64) * 2
    for i in range(nq):
        ctx[2 * i] += (plant * q[i] / np.linalg.norm(q[i])).astype(np.float32)
    if nq > max(INBATCH_DUP_ROWS):
        hi, lo = INBATCH_DUP_ROWS
        ctx[2 * hi + 1] = ctx[2 * hi]
        ctx[2 * lo - 1] = ctx[2 * lo]
    return q, ctx, pos


def scores_fp64(q, ctx):
    """q ctx^T in fp64 where identical rows of ctx give identical columns whatever BLAS does with a column's position: the product
    is taken over the distinct rows and expanded."""
    q, ctx = np.asarray(q, np.float64), np.asarray(ctx, np.float64)
    uniq, inv = np.unique(ctx, axis=0, return_inverse=True)
    return (q @ uniq.T)[:, np.asarray(inv).reshape(-1)]


def inbatch_margins(q, ctx, pos):
    """fp64 lead of every row's best score over the best DIFFERENT score (duplicated columns tie exactly and are not a margin)."""
    s = scores_fp64(q, ctx)
    out = np.empty(len(s))
    for i, row in enumerate(s):
        top = row.max()
        rest = row[row != top]
        out[i] = top - rest.max() if rest.size else np.inf
    return out


# ---------------------------------------------------------------------------------------------------------------- oracles
def nll_fp64(q, a, b, mask_a=None, mask_b=None, grad_output=1.0):
    """dict(loss, logits [n, 2], ca, cb, gq, ga, gb) in fp64.  The winner of the max over chunks is the LOWEST index among equal
    biased scores (np.argmax)."""
    q, a, b = (np.asarray(x, np.float64) for x in (q, a, b))
    n = q.shape[0]
    firstp = a.ndim == 2
    if firstp:
        a, b = a[:, None, :], b[:, None, :]
        mask_a = mask_b = np.ones((n, 1))
    # row-wise sums, not BLAS: two identical chunk rows must give identical scores (the tie the lowest index wins)
    sa = (q[:, None, :] * a).sum(-1) + (1.0 - np.asarray(mask_a, np.float64)) * -9999.0
    sb = (q[:, None, :] * b).sum(-1) + (1.0 - np.asarray(mask_b, np.float64)) * -9999.0
    ca, cb = sa.argmax(1), sb.argmax(1)
    r = np.arange(n)
    la, lb = sa[r, ca], sb[r, cb]
    x = lb - la
    loss = float(np.mean(np.logaddexp(0.0, x)))
    p = np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))
    s = grad_output / n
    dla, dlb = -p * s, p * s
    gq = dla[:, None] * a[r, ca] + dlb[:, None] * b[r, cb]
    ga, gb = np.zeros_like(a), np.zeros_like(b)
    ga[r, ca] = dla[:, None] * q
    gb[r, cb] = dlb[:, None] * q
    if firstp:
        ga, gb = ga[:, 0], gb[:, 0]
    return dict(loss=loss, logits=np.stack([la, lb], 1), ca=ca, cb=cb, gq=gq, ga=ga, gb=gb)


def inbatch_fp64(q, ctx, pos, grad_output=1.0):
    """dict(loss, correct [nq] bool, n_correct, gq, gctx, scores) in fp64; argmax = the lowest column among equal scores."""
    q, ctx = np.asarray(q, np.float64), np.asarray(ctx, np.float64)
    pos = np.asarray(pos)
    nq = q.shape[0]
    s = scores_fp64(q, ctx)
    m = s.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(s - m).sum(1))
    r = np.arange(nq)
    loss = float(np.mean(lse - s[r, pos]))
    correct = s.argmax(1) == pos
    g = np.exp(s - lse[:, None])
    g[r, pos] -= 1.0
    g *= grad_output / nq
    return dict(loss=loss, correct=correct, n_correct=int(correct.sum()), gq=g @ ctx, gctx=g.T @ q, scores=s)


def clip_fp64(grads, max_norm):
    """(total 2-norm, coef) of clip_grad_norm_ over the given gradients in fp64 (the 1e-6 is the fp32 constant)."""
    total = math.sqrt(sum(float(np.dot(np.asarray(g, np.float64).ravel(), np.asarray(g, np.float64).ravel())) for g in grads))
    return total, min(max_norm / (total + U.f32(1e-6)), 1.0)


def run_clipped_fp64(max_norm, steps=CLIP_STEPS):
    """tests/lamb_util.py's fixture with clip_grad_norm_(max_norm) in front of every step, in fp64:
    [(total_norm, coef, {name: (p, m, v, wn, an, tr)})] per step."""
    P = U.init_params()
    state = {n: (P[n].astype(np.float64), np.zeros(P[n].shape), np.zeros(P[n].shape)) for n in P}
    out = []
    for t in range(steps):
        grads = {name: U.grad(name, t) for name, *_ in U.SPEC}
        total, coef = clip_fp64([g for g in grads.values() if g is not None], max_norm)
        rec = {}
        for name, shape, gi, _, _ in U.SPEC:
            if grads[name] is None:
                continue
            p, m, v = state[name]
            r = U.step_fp64(p, grads[name].astype(np.float64) * coef, m, v, U.group_lr(gi, t), U.BETAS, U.EPS,
                            U.GROUPS[gi]["weight_decay"], False)
            state[name] = r[:3]
            rec[name] = r
        out.append((total, coef, rec))
    return out


def bound(ref_err, scale):
    """The bound of tests/test_gpu_lamb.py:78-86: max(4 x the reference's own max |delta| from fp64, 2 ulp of the tensor's largest
    magnitude)."""
    return max(4.0 * float(ref_err), 2.0 * U.ulp32(scale))
