"""The 16-bit BertLayer seams (ance_amd/layers.py precision="half" -> csrc/layer_tail_half.hip) restated for their tests, on top of
layer_tail_util:

  round16            float64 / float32 values rounded ONCE to fp16 / bf16 in NumPy integer arithmetic: to nearest, ties to even, the
                     subnormals included, overflow to +-inf (never clamped), NaN kept.  Returned as float64 (every 16-bit value is
                     exact there).  tests/test_layer_half.py pins it to torch's own .to(dtype).
  ulp16              the dtype's spacing at |x|, elementwise (the subnormal spacing below the smallest normal)
  tail16_fp64 / gelu16_fp64   the two seams of include/ance_amd.h in fp64 on 16-bit-valued inputs: layer_tail_util's fp64 seams with
                     g = dy + dy16, plus the 16-bit outputs rounded once (y16, and the T-typed dx / y)
  within16           the 16-bit outputs' bound, elementwise: |got - want| <= ulp16(max(|got|, |want|)) / 2 + B32, B32 the fp32 seams'
                     bound for that tensor (layer_tail_util.bound): the fp32 arithmetic may be B32 off, the store rounds once more
"""
import numpy as np

import layer_tail_util as U

FORMATS = {"fp16": (10, -14, 15), "bf16": (7, -126, 127)}   # explicit mantissa bits, smallest normal exponent, largest exponent
DTYPES = ("fp16", "bf16")


def torch_dtype(name):
    import torch
    return {"fp16": torch.float16, "bf16": torch.bfloat16}[name]


def round16(x, name):
    """x rounded once to the format, as float64.  Exact: x is scaled by a power of two so that the format's spacing at |x| becomes 1
    (exact in fp64 for every fp32 and every fp64 of an fp32-sized exponent), rounded with np.rint (ties to even) and scaled back."""
    mant, emin, emax = FORMATS[name]
    x = np.asarray(x, np.float64)
    a = np.abs(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.floor(np.log2(np.where((a > 0) & np.isfinite(a), a, 1.0)))
    # log2 of a value just below a power of two may round up to it: step back where 2^e > a
    e = np.where(np.ldexp(1.0, e.astype(np.int64)) > a, e - 1, e)
    e = np.maximum(e, emin).astype(np.int64)
    q = np.ldexp(np.rint(np.ldexp(a, -(e - mant))), e - mant)      # may carry into the next binade: still a value of the format
    big = np.ldexp(2.0 - 2.0 ** -mant, emax)                       # the largest finite value
    q = np.where(q > big, np.inf, q)
    out = np.where(np.isfinite(a), np.copysign(q, x), x)           # +-inf and NaN pass
    return out


def ulp16(x, name):
    mant, emin, _ = FORMATS[name]
    a = np.abs(np.asarray(x, np.float64))
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    e = np.where(np.ldexp(1.0, e.astype(np.int64)) > a, e - 1, e)
    e = np.maximum(np.where(a > 0, e, emin), emin).astype(np.int64)
    return np.ldexp(1.0, e - mant)


def rounded(x, name):
    """fp32 array holding the format's values: what the kernels and the fp64 truth both see."""
    return None if x is None else round16(x, name).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ the seams
def tail16_fp64(x, bias, res, gamma, beta, eps, dy, dy16, name, keep=None, p=0.0):
    """x holds the format's values; dy (fp32-valued) and dy16 (format-valued) are each optional.  layer_tail_util.tail_fp64's dict
    on g = dy + dy16, plus y16 = round16(y) and dx16 = round16(dx)."""
    g = (0.0 if dy is None else np.asarray(dy, np.float64)) + (0.0 if dy16 is None else np.asarray(dy16, np.float64))
    r = U.tail_fp64(x, bias, res, gamma, beta, eps, g, keep, p)
    r["y16"], r["dx16"] = round16(r["y"], name), round16(r["dx"], name)
    return r


def gelu16_fp64(x, bias, dy, name):
    r = U.gelu_fp64(x, bias, dy)
    r["y16"], r["dx16"] = round16(r["y"], name), round16(r["dx"], name)
    return r


def eager_layer(hs, rows, W, nh, eps):
    """transformers' eager BertLayer with torch ops (dropout 0), ctx zeroed at pad rows as ance_amd.layers.BertLayer leaves it: under
    torch.autocast this is the layer whose own distance D from the fp32 BertLayer sets the layer-level bound."""
    import torch
    F = torch.nn.functional
    B, L, H = hs.shape

    def heads(x):
        return x.view(B, L, nh, 64).permute(0, 2, 1, 3)

    def lin(x, name):
        return F.linear(x, W[name + ".weight"], W[name + ".bias"])

    q, k, v = (lin(hs, "attention.self." + n) for n in ("query", "key", "value"))
    mask = ((1.0 - rows.float()) * -10000.0)[:, None, None, :]
    probs = torch.softmax(torch.matmul(heads(q), heads(k).transpose(-1, -2)) / 8.0 + mask, dim=-1)
    ctx = torch.matmul(probs, heads(v)).permute(0, 2, 1, 3).contiguous().view(B, L, H)
    ctx = ctx * rows[:, :, None].to(ctx.dtype)
    ln = "attention.output.LayerNorm"
    h = F.layer_norm(lin(ctx, "attention.output.dense") + hs, (H,), W[ln + ".weight"], W[ln + ".bias"], eps)
    t = lin(h, "intermediate.dense")
    t = t * 0.5 * (1.0 + torch.erf(t / 1.4142135623730951))
    ln = "output.LayerNorm"
    return F.layer_norm(lin(t, "output.dense") + h, (H,), W[ln + ".weight"], W[ln + ".bias"], eps)


def within16(got, want, b32, name):
    """(ok, worst excess ratio): elementwise |got - want| <= ulp16(max(|got|, |want|)) / 2 + b32, want the UNROUNDED fp64 tensor."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    lim = 0.5 * ulp16(np.maximum(np.abs(got), np.abs(want)), name) + b32
    d = np.abs(got - want)
    return bool(np.all(d <= lim)), float((d / lim).max())
