"""The trainers' self-attention core (ance_amd/attention.py -> csrc/attention_train.hip) restated for its tests:

  attention_fp64     fp64 NumPy on the padded form, with the reference's additive -10000 mask and an explicit keep mask
  philox4x32 / keep_mask   the dropout stream of include/ance_amd.h restated (Philox4x32-10, known answers in PHILOX_KAT)
  eager_fp32         transformers' eager expression in torch fp32 on the CPU (matmul, / 8, mask add, softmax, dropout, matmul) with
                     its autograd gradients: the reference whose own distance from fp64 sets the tests' bound
  tiled_fp32         an fp32 NumPy restatement in the kernels' own order (32-key blocks, online softmax, recomputed P, one owner
                     per dK / dV / dQ tile): what a re-ordered fp32 evaluation costs, measured on the CPU
  bound              max(4 x the reference's distance, 16 ulp32 of the fp64 tensor's largest magnitude)
"""
import numpy as np

from oracle.encoder_ref import det_normal

HEAD = 64
NAMES = ("ctx", "lse", "dq", "dk", "dv")
SWEEP_LENS = (129, 1, 512, 64, 2, 257, 63, 511, 128, 65, 255, 127, 256)   # the issue's lengths, shuffled
SWEEP_LENS_16 = (65, 512, 1, 257, 128, 63)
DROPOUT_LENS = (1, 5, 64, 130)
GOLDEN_CASES = ("rdot", "bert")

PHILOX_KAT = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def ulp32(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def bound(ref_err, largest):
    return max(4.0 * float(ref_err), 16.0 * ulp32(largest))


# ------------------------------------------------------------------------------------------------------------------ Philox
def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint32 arrays (broadcast): the four output words."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(0xFFFFFFFF) for x in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    M0, M1, mask = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        hi0, lo0, hi1, lo1 = p0 >> s32, p0 & mask, p1 >> s32, p1 & mask
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def keep_threshold(p):
    return int(np.floor(float(np.float32(p)) * 4294967296.0))


def keep_mask(p, seed, offset, s, h, n_heads, n_q, n_k):
    """bool [n_q, n_k]: the keys that query i of head h of sequence index s keeps under (seed, offset)."""
    i = np.arange(n_q, dtype=np.uint64)[:, None]
    j4 = np.arange((n_k + 3) // 4, dtype=np.uint64)[None, :]
    w = philox4x32(i * np.uint64(128) + j4, s * n_heads + h, offset & 0xFFFFFFFF, offset >> 32, seed & 0xFFFFFFFF, seed >> 32)
    words = np.stack(w, axis=-1).reshape(n_q, -1)[:, :n_k]
    return words >= np.uint32(keep_threshold(p)) if keep_threshold(p) > 0 else np.ones((n_q, n_k), bool)


def keep_masks(p, seed, offset, lens, n_heads, L):
    """bool [B, n_heads, L, L] for a padded call (sequence index = batch row)."""
    return np.stack([np.stack([keep_mask(p, seed, offset, s, h, n_heads, L, L) for h in range(n_heads)]) for s in range(len(lens))])


# ------------------------------------------------------------------------------------------------------------------ inputs
def seeded_inputs(tag, lens, n_heads, L=None, q_scale=1.0, seed=31):
    """q, k, v, dctx [B, L, 64 n_heads] fp32 (every row filled, pad rows included) and lens."""
    lens = np.asarray(lens, dtype=np.int32)
    L = int(L or lens.max())
    shape = (len(lens), L, HEAD * n_heads)
    q = det_normal(seed, tag + ".q", shape, 1.0) * np.float32(q_scale)
    return q, det_normal(seed, tag + ".k", shape, 1.0), det_normal(seed, tag + ".v", shape, 1.0), det_normal(seed, tag + ".g", shape, 0.1), lens


def pack(x, lens):
    """[B, L, H] -> the valid rows [sum lens, H] and seq_off."""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return np.concatenate([x[b, :n] for b, n in enumerate(lens)], axis=0), off


def unpack(x, lens, L):
    out = np.zeros((len(lens), L) + x.shape[1:], dtype=x.dtype)
    o = 0
    for b, n in enumerate(lens):
        out[b, :n] = x[o:o + n]
        o += n
    return out


def _heads(x, n_heads):
    B, L, _ = x.shape
    return x.reshape(B, L, n_heads, HEAD).transpose(0, 2, 1, 3)


def _merge(x):
    B, nh, L, _ = x.shape
    return x.transpose(0, 2, 1, 3).reshape(B, L, nh * HEAD)


def _valid(lens, L):
    return np.arange(L)[None, :] < np.asarray(lens)[:, None]


# ------------------------------------------------------------------------------------------------------------------ fp64
def attention_fp64(q, k, v, dctx, lens, n_heads, keep=None, p=0.0):
    """The padded form in fp64 with the additive -10000 mask on pad keys.  keep: bool [B, n_heads, L, L] or None.  Pad query rows: dctx
    is ignored there and ctx, lse and the gradients are zeros.  Returns dict(ctx, lse [n_heads, B * L], dq, dk, dv)."""
    B, L, _ = q.shape
    rows = _valid(lens, L)
    Q, K, V = (_heads(np.asarray(x, np.float64), n_heads) for x in (q, k, v))
    G = _heads(np.where(rows[:, :, None], np.asarray(dctx, np.float64), 0.0), n_heads)
    S = Q @ K.transpose(0, 1, 3, 2) * 0.125 + ((1.0 - rows.astype(np.float64)) * -10000.0)[:, None, None, :]
    m = S.max(-1, keepdims=True)
    E = np.exp(S - m)
    Z = E.sum(-1, keepdims=True)
    P = E / Z
    lse = (m + np.log(Z))[..., 0]
    scale = 1.0 / (1.0 - float(np.float32(p))) if keep is not None else 1.0
    Pd = P * keep * scale if keep is not None else P
    ctx = Pd @ V
    dV = Pd.transpose(0, 1, 3, 2) @ G
    dP = G @ V.transpose(0, 1, 3, 2)
    if keep is not None:
        dP = dP * keep * scale
    dS = P * (dP - (dP * P).sum(-1, keepdims=True))
    dQ, dK = dS @ K * 0.125, dS.transpose(0, 1, 3, 2) @ Q * 0.125
    z = rows[:, :, None]
    out = dict(ctx=np.where(z, _merge(ctx), 0.0), dq=np.where(z, _merge(dQ), 0.0), dk=np.where(z, _merge(dK), 0.0),
               dv=np.where(z, _merge(dV), 0.0))
    out["lse"] = np.where(rows[:, None, :], lse, 0.0).transpose(1, 0, 2).reshape(n_heads, B * L)
    return out


# ------------------------------------------------------------------------------------------------------------------ torch eager fp32
def eager_fp32(q, k, v, dctx, lens, n_heads, keep=None, p=0.0):
    """transformers' eager expression (BertSelfAttention.forward of 2.3.0) in torch fp32 on the CPU, the dropout given as a mask;
    gradients by autograd with dctx zeroed at pad rows.  Same dict as attention_fp64, fp32, pad rows zeroed."""
    import math

    import torch
    B, L, H = q.shape
    rows = _valid(lens, L)
    tq, tk, tv = (torch.from_numpy(np.array(x, np.float32)).requires_grad_(True) for x in (q, k, v))

    def tfs(x):
        return x.view(B, L, n_heads, HEAD).permute(0, 2, 1, 3)

    mask = torch.from_numpy(((1.0 - rows.astype(np.float32)) * -10000.0))[:, None, None, :]
    scores = torch.matmul(tfs(tq), tfs(tk).transpose(-1, -2)) / math.sqrt(HEAD) + mask
    probs = torch.softmax(scores, dim=-1)
    if keep is not None:
        probs = probs * torch.from_numpy(keep.astype(np.float32)) * (1.0 / (1.0 - float(np.float32(p))))
    ctx = torch.matmul(probs, tfs(tv)).permute(0, 2, 1, 3).contiguous().view(B, L, H)
    g = torch.from_numpy(np.where(rows[:, :, None], np.asarray(dctx, np.float32), np.float32(0)))
    ctx.backward(g)
    lse = torch.logsumexp(scores.detach(), dim=-1).numpy()
    z = rows[:, :, None]
    out = dict(ctx=np.where(z, ctx.detach().numpy(), 0), dq=np.where(z, tq.grad.numpy(), 0), dk=np.where(z, tk.grad.numpy(), 0),
               dv=np.where(z, tv.grad.numpy(), 0))
    out["lse"] = np.where(rows[:, None, :], lse, 0).transpose(1, 0, 2).reshape(n_heads, B * L)
    return out


def distances(got, want):
    return {n: float(np.abs(np.asarray(got[n], np.float64) - want[n]).max()) for n in NAMES}


# ------------------------------------------------------------------------------------------------------------------ the kernels' order
def tiled_fp32(q, k, v, dctx, n, keep=None, p=0.0, blk=32):
    """One head of one sequence ([L, 64] fp32 each, n valid rows) in fp32 in the kernels' order: the forward walks 32-key blocks with an
    online softmax and divides at the end; the backward recomputes P = exp(S - lse) per 32 x 32 block, D = dctx . ctx, and sums the
    blocks' contributions in ascending order.  Returns (ctx, lse, dq, dk, dv) for the n valid rows."""
    f = np.float32
    q, k, v, g = (np.asarray(x[:n], f) for x in (q, k, v, dctx))
    keep = None if keep is None else keep[:n, :n]
    rs = f(1.0) / (f(1.0) - f(p)) if keep is not None else f(1.0)
    qs = q * f(0.125)
    # The scores are formed once: the kernels' backward recomputes them in the forward's own order, bit for bit (the same fmaf
    # chain over d), and that matters -- with scores that differ in the last bits between the passes (two BLAS calls of different
    # shapes here), P = exp(S - lse) of a saturated row is off by ulp(S) where the eager softmax is exact, and dv measured 3.4 - 5.4 x
    # the eager expression's distance at score scales 8 and 30; with one S it is 0.5 - 1.2 x at scales 1, 8, 30.
    S = qs @ k.T
    m, l, acc = np.full(n, -np.inf, f), np.zeros(n, f), np.zeros((n, HEAD), f)
    for j0 in range(0, n, blk):
        s = S[:, j0:j0 + blk]
        mn = np.maximum(m, s.max(-1))
        alpha = np.exp(m - mn, dtype=f)
        e = np.exp(s - mn[:, None], dtype=f)
        l = l * alpha + e.sum(-1, dtype=f)
        if keep is not None:
            e = np.where(keep[:, j0:j0 + blk], e, f(0))
        acc = acc * alpha[:, None] + e @ v[j0:j0 + blk]
        m = mn
    ctx = acc * (rs / l)[:, None]
    lse = m + np.log(l, dtype=f)
    D = (g * ctx).sum(-1, dtype=f)
    dq, dk, dv = np.zeros((n, HEAD), f), np.zeros((n, HEAD), f), np.zeros((n, HEAD), f)
    for j0 in range(0, n, blk):
        for i0 in range(0, n, blk):
            pb = np.exp(S[i0:i0 + blk, j0:j0 + blk] - lse[i0:i0 + blk, None], dtype=f)
            dp = g[i0:i0 + blk] @ v[j0:j0 + blk].T
            pk = pb
            if keep is not None:
                kb = keep[i0:i0 + blk, j0:j0 + blk]
                dp, pk = np.where(kb, dp * rs, f(0)), np.where(kb, pb * rs, f(0))
            ds = pb * (dp - D[i0:i0 + blk, None])
            dv[j0:j0 + blk] += pk.T @ g[i0:i0 + blk]
            dk[j0:j0 + blk] += ds.T @ q[i0:i0 + blk]
            dq[i0:i0 + blk] += ds @ k[j0:j0 + blk]
    return ctx, lse, dq * f(0.125), dk * f(0.125), dv
