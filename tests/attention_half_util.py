"""The 16-bit attention core (ance_amd/attention.py precision="half" -> csrc/attention_train_half.hip) restated for its tests, on top of
attention_train_util:

  round16            fp32 values rounded to fp16 / bf16 (to nearest even), kept as fp32: what the fp64 truth and the kernels both see
  eager_half         the eager autocast expression on the CPU: every matmul is (a.float() @ b.float()) rounded to the dtype, the
                     scaling and the mask add are rounded to the dtype, softmax is fp32, the probabilities are rounded to the dtype
                     before the second matmul; gradients by autograd through those roundings.  Its own distance from fp64 sets the bound
  kernel_model_half  the arithmetic contract of the kernels' header comment in numpy/torch: 32-key online softmax, hardware-style
                     exp2(x log2 e), P' and dS rounded to the dtype, fp32 accumulation, one rounding at each store
  ulp16 / bound16    bound16 = max(4 x the reference's distance, 2 ulp of the dtype at the fp64 tensor's largest magnitude): the 4 x is
                     the project's margin, the 2 ulp floor covers the store rounding plus the operand roundings
"""
import numpy as np
import torch

import attention_train_util as A

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
LOG2E = np.float32(1.4426950408889634)


def round16(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dtype).float().numpy()


def ulp16(x, dtype):
    """One ulp of dtype at |x| (the spacing above the power of two below it; the subnormal spacing under the smallest normal)."""
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    x = abs(float(x))
    e = emin if x == 0.0 else max(int(np.floor(np.log2(x))), emin)
    return 2.0 ** (e - mant)


def bound16(ref_err, largest, dtype):
    return max(4.0 * float(ref_err), 2.0 * ulp16(largest, dtype))


def rounded_inputs(tag, lens, n_heads, dtype, L=None, q_scale=1.0, g_scale=1.0):
    """A.seeded_inputs rounded to dtype first (fp32 arrays holding 16-bit values), so that fp64 sees what the kernels see."""
    q, k, v, g, ln = A.seeded_inputs(tag, lens, n_heads, L=L, q_scale=q_scale)
    return round16(q, dtype), round16(k, dtype), round16(v, dtype), round16(g * np.float32(g_scale), dtype), ln


def eager_half(q, k, v, dctx, lens, n_heads, dtype, keep=None, p=0.0):
    """Same dict as A.attention_fp64 (fp32 arrays, pad rows zeroed); lse from the dtype-rounded masked scores in fp32."""
    B, L, H = q.shape
    rows = A._valid(lens, L)
    tq, tk, tv = (torch.from_numpy(np.array(x, np.float32)).to(dtype).requires_grad_(True) for x in (q, k, v))

    def tfs(x):
        return x.view(B, L, n_heads, A.HEAD).permute(0, 2, 1, 3)

    def mm(a, b):
        return (a.float() @ b.float()).to(dtype)

    mask = torch.from_numpy(((1.0 - rows.astype(np.float32)) * -10000.0))[:, None, None, :].to(dtype)
    scores = mm(tfs(tq), tfs(tk).transpose(-1, -2)) / 8.0 + mask
    probs = torch.softmax(scores.float(), dim=-1)
    if keep is not None:
        probs = probs * torch.from_numpy(keep.astype(np.float32)) * (1.0 / (1.0 - float(np.float32(p))))
    ctx = mm(probs.to(dtype), tfs(tv)).permute(0, 2, 1, 3).contiguous().view(B, L, H)
    g = torch.from_numpy(np.where(rows[:, :, None], np.asarray(dctx, np.float32), np.float32(0))).to(dtype)
    ctx.backward(g)
    lse = torch.logsumexp(scores.detach().float(), dim=-1).numpy()
    z = rows[:, :, None]
    out = dict(ctx=np.where(z, ctx.detach().float().numpy(), 0), dq=np.where(z, tq.grad.float().numpy(), 0),
               dk=np.where(z, tk.grad.float().numpy(), 0), dv=np.where(z, tv.grad.float().numpy(), 0))
    out["lse"] = np.where(rows[:, None, :], lse, 0).transpose(1, 0, 2).reshape(n_heads, B * L)
    return out


def _ex(x):
    """The kernels' exp: exp2 of the fp32 product x * log2 e."""
    with np.errstate(invalid="ignore", over="ignore"):   # masked-out arguments may overflow; np.where drops them
        return np.exp2((x.astype(np.float32) * LOG2E).astype(np.float32)).astype(np.float32)


def kernel_model_half(q, k, v, dctx, lens, n_heads, dtype, keep=None, p=0.0, blk=32):
    """The contract of csrc/attention_train_half.hip on the padded form (inputs: fp32 arrays holding dtype values).  Same dict as
    A.attention_fp64, fp32 arrays holding dtype values (lse fp32), pad rows zeroed."""
    f = np.float32
    B, L, _ = q.shape
    lens = np.asarray(lens)
    rows = A._valid(lens, L)
    Q, K, V = (A._heads(np.asarray(x, f), n_heads) for x in (q, k, v))
    G = A._heads(np.where(rows[:, :, None], np.asarray(dctx, f), f(0)), n_heads)
    kmask = rows[:, None, None, :]
    rs = f(1.0) / (f(1.0) - f(p)) if keep is not None else f(1.0)
    T = np.where(kmask, (Q @ K.transpose(0, 1, 3, 2)) * f(0.125), f(-np.inf)).astype(f)   # 16-bit products are exact in fp32
    m = np.full((B, n_heads, L), -np.inf, f)
    l = np.zeros((B, n_heads, L), f)
    acc = np.zeros((B, n_heads, L, A.HEAD), f)
    with np.errstate(invalid="ignore"):
        for j0 in range(0, int(lens.max()), blk):
            t = T[..., j0:j0 + blk]
            mn = np.maximum(m, t.max(-1))
            safe = np.where(np.isfinite(mn), mn, f(0))
            alpha = np.where(np.isfinite(m), _ex(m - safe), f(0))
            e = _ex(t - safe[..., None])
            l = l * alpha + e.sum(-1, dtype=f)
            if keep is not None:
                e = np.where(keep[..., j0:j0 + blk], e, f(0))
            acc = acc * alpha[..., None] + round16(e, dtype) @ V[:, :, j0:j0 + blk]
            m = mn
    ok = rows[:, None, :]
    lsafe = np.where(ok & (l > 0), l, f(1))
    ctx = round16(acc * (rs / lsafe)[..., None], dtype)
    lse = np.where(ok, np.where(np.isfinite(m), m, f(0)) + np.log(lsafe, dtype=f), f(0)).astype(f)
    D = (G * ctx).sum(-1, dtype=f)
    P = np.where(kmask & ok[..., None], _ex(np.where(kmask, T, f(0)) - lse[..., None]), f(0)).astype(f)
    dP = G @ V.transpose(0, 1, 3, 2)
    Pk = P
    if keep is not None:
        dP, Pk = np.where(keep, dP * rs, f(0)), np.where(keep, P * rs, f(0))
    with np.errstate(over="ignore", invalid="ignore"):
        dS = round16(P * (dP - D[..., None]), dtype)
        Pk = round16(Pk, dtype)
        dq = round16((dS @ K) * f(0.125), dtype)
        dk = round16((dS.transpose(0, 1, 3, 2) @ Q) * f(0.125), dtype)
        dv = round16(Pk.transpose(0, 1, 3, 2) @ G, dtype)
    z = rows[:, :, None]
    out = dict(ctx=np.where(z, A._merge(ctx), f(0)), dq=np.where(z, A._merge(dq), f(0)), dk=np.where(z, A._merge(dk), f(0)),
               dv=np.where(z, A._merge(dv), f(0)))
    out["lse"] = lse.transpose(1, 0, 2).reshape(n_heads, B * L)
    return out


def bounds(ref_err, want, dtype):
    """Per tensor: bound16 for the 16-bit tensors, A.bound for the fp32 log-sum-exp."""
    return {n: (A.bound(ref_err[n], np.abs(want[n]).max()) if n == "lse" else bound16(ref_err[n], np.abs(want[n]).max(), dtype))
            for n in A.NAMES}


def check(tag, got, want, ref_err, dtype, names=A.NAMES):
    """Prints every measured distance and ratio, then asserts them all."""
    b = bounds(ref_err, want, dtype)
    bad = []
    for n in names:
        d = float(np.abs(np.asarray(got[n], np.float64) - want[n]).max())
        print("%-34s %-4s max|delta| %.3e  eager_half %.3e  ratio %5.2f  bound %.3e" % (tag, n, d, ref_err[n], d / max(ref_err[n], 1e-300), b[n]))
        if not d <= b[n]:
            bad.append((n, d, b[n]))
    assert not bad, (tag, bad)


# the seeded cases the GPU file runs within bound16: (tag, lens, n_heads, L, q_scale, p); the CPU file pins the model on each
SEEDED_CASES = (
    ("dropout", A.DROPOUT_LENS, 12, 130, 1.0, 0.1),
    ("dropout", A.DROPOUT_LENS, 12, 130, 1.0, 0.5),
    ("saturated.8", (33, 97), 12, 97, 8.0, 0.0),
    ("saturated.30", (33, 97), 12, 97, 30.0, 0.0),
    ("layouts", (96, 31, 0), 12, 96, 1.0, 0.0),
    ("vs32", (70, 33, 128), 12, 128, 1.0, 0.0),
)
DROPOUT_SEED = 0x5EED0123456789AB


def seeded_reference(tag, lens, nh, L, q_scale, p, seed, offset, dtype_name, g_scale=1.0):
    """Inputs (dtype-valued), the fp64 restatement and eager_half's distances for one seeded case on the padded form."""
    dtype = DTYPES[dtype_name]
    q, k, v, g, ln = rounded_inputs(tag, lens, nh, dtype, L=L, q_scale=q_scale, g_scale=g_scale)
    keep = A.keep_masks(p, seed, offset, ln, nh, q.shape[1]) if p > 0 else None
    want = A.attention_fp64(q, k, v, g, ln, nh, keep, p)
    ref = A.distances(eager_half(q, k, v, g, ln, nh, dtype, keep, p), want)
    return (q, k, v, g, ln), want, ref, keep


def sweep_reference(lens, nh, dtype_name):
    """The length sweep: every sequence restated on its own (L = its length), results laid into the padded form."""
    dtype = DTYPES[dtype_name]
    q, k, v, g, ln = rounded_inputs("sweep.%d" % nh, lens, nh, dtype)
    L = q.shape[1]
    want = {n: np.zeros((len(lens), L, 64 * nh)) for n in ("ctx", "dq", "dk", "dv")}
    want["lse"] = np.zeros((nh, len(lens) * L))
    ref = {n: 0.0 for n in A.NAMES}
    for b, n in enumerate(lens):
        one = [x[b:b + 1, :n] for x in (q, k, v, g)]
        w = A.attention_fp64(*one, [n], nh)
        for name, d in A.distances(eager_half(*one, [n], nh, dtype), w).items():
            ref[name] = max(ref[name], d)
        for name in ("ctx", "dq", "dk", "dv"):
            want[name][b, :n] = w[name][0]
        want["lse"][:, b * L:b * L + n] = w["lse"]
    return (q, k, v, g, ln), want, ref


def one_hot_case(n, seed=7):
    """One sequence of length n, 12 heads, small integers: k_j encodes j in +-8 over 9 bit positions, each repeated 7 times across the 64
    columns (the last column is 0); q_i encodes pi(i) the same way.  The score of (i, j) is 0.125 * 64 * 7 * (9 - 2 hamming(pi(i), j)):
    the winner beats every other key by >= 112, so P is exactly one-hot in fp32 (exp(-112) is below half an ulp of 1 and rounds to 0
    in 16 bits).  v, dctx: integers in -4 .. 4.  Returns q, k, v, dctx [1, n, 768] fp32 and pi [12, n] (a permutation per head)."""
    rng = np.random.RandomState(seed + n)
    nh = 12
    bits = ((np.arange(n)[:, None] >> np.arange(9)[None, :]) & 1) * 2 - 1            # [n, 9] in +-1
    code = np.concatenate([np.repeat(bits, 7, axis=1) * 8, np.zeros((n, 1), int)], axis=1).astype(np.float32)   # [n, 64]
    pi = np.stack([rng.permutation(n) for _ in range(nh)])
    q = np.concatenate([code[pi[h]] for h in range(nh)], axis=1)[None]
    k = np.concatenate([code] * nh, axis=1)[None]
    v = rng.randint(-4, 5, size=(1, n, 64 * nh)).astype(np.float32)
    g = rng.randint(-4, 5, size=(1, n, 64 * nh)).astype(np.float32)
    return q, k, v, g, pi
