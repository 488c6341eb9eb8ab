"""The row-wise seams of a BertLayer (ance_amd/layers.py -> csrc/layer_tail.hip) restated for their tests:

  tail_fp64 / gelu_fp64        fp64 NumPy, forward and backward, the dropout given as an explicit keep mask
  tail_keep_mask               the keep mask of include/ance_amd.h's counter (row, col >> 2, offset lo, offset hi), word col & 3
  tail_eager_fp32 / gelu_eager_fp32   transformers' eager expressions in torch fp32 on the CPU with their autograd gradients: the
                               reference whose own distance from fp64 sets the tests' bound (attention_train_util.bound)
  layer_fp64 / layer_torch     a whole BertLayer as ance_amd.layers.BertLayer composes it (pad rows of the attention's context are
                               zeros), in fp64 NumPy from attention_train_util.attention_fp64 and the two above, and in torch on the CPU
  layer_torch_forward          layer_torch's forward on torch tensors, in the graph: what tests/train_step_util.py chains into a tower
"""
import math

import numpy as np

import attention_train_util as A
from oracle.encoder_ref import det_normal

bound = A.bound
TAIL_NAMES = ("y", "dx", "dres", "dgamma", "dbeta", "dbias")
GELU_NAMES = ("y", "dx", "dbias")
GOLDEN_CASES = A.GOLDEN_CASES
SEAMS = ("attention.output", "output", "intermediate")
LAYER_PARAMS = tuple("%s.%s" % (m, w) for m in ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense",
                                                 "attention.output.LayerNorm", "intermediate.dense", "output.dense", "output.LayerNorm")
                     for w in ("weight", "bias"))


def _scale(p):
    return 1.0 / (1.0 - float(np.float32(p)))


# ------------------------------------------------------------------------------------------------------------------ the mask
def tail_keep_mask(p, seed, offset, n_rows, H):
    """bool [n_rows, H]: the columns that row r keeps under (seed, offset)."""
    thr = A.keep_threshold(p)
    if thr == 0:
        return np.ones((n_rows, H), bool)
    r = np.arange(n_rows, dtype=np.uint64)[:, None]
    c4 = np.arange(H // 4, dtype=np.uint64)[None, :]
    w = A.philox4x32(r, c4, offset & 0xFFFFFFFF, offset >> 32, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(w, axis=-1).reshape(n_rows, H) >= np.uint32(thr)


# ------------------------------------------------------------------------------------------------------------------ fp64
def tail_fp64(x, bias, res, gamma, beta, eps, dy, keep=None, p=0.0):
    """[n_rows, H] each.  dict(y, dx, dres, dgamma, dbeta, dbias); dbias is None without a bias."""
    x, res, gamma, beta, dy = (np.asarray(t, np.float64) for t in (x, res, gamma, beta, dy))
    H = x.shape[-1]
    u = x + (np.asarray(bias, np.float64) if bias is not None else 0.0)
    k = keep * _scale(p) if keep is not None else 1.0
    z = u * k + res
    mean = z.mean(-1, keepdims=True)
    var = ((z - mean) ** 2).sum(-1, keepdims=True) / H
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (z - mean) * rstd
    g = dy * gamma
    dz = rstd * (g - g.mean(-1, keepdims=True) - xhat * (g * xhat).mean(-1, keepdims=True))
    dx = dz * k
    return dict(y=xhat * gamma + beta, dx=dx, dres=dz, dgamma=(dy * xhat).sum(0), dbeta=dy.sum(0),
                dbias=dx.sum(0) if bias is not None else None)


def _erf64(z):
    return np.vectorize(math.erf, otypes=[np.float64])(z)


def gelu_fp64(x, bias, dy):
    u = np.asarray(x, np.float64) + np.asarray(bias, np.float64)
    cdf = 0.5 * (1.0 + _erf64(u / math.sqrt(2.0)))
    dx = np.asarray(dy, np.float64) * (cdf + u * np.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi))
    return dict(y=u * cdf, dx=dx, dbias=dx.sum(0))


# ------------------------------------------------------------------------------------------------------------------ torch eager fp32
def _t(x, grad=True):
    import torch
    t = torch.from_numpy(np.array(x, np.float32))
    return t.requires_grad_(True) if grad else t


def tail_eager_fp32(x, bias, res, gamma, beta, eps, dy, keep=None, p=0.0):
    """BertSelfOutput / BertOutput after the dense matmul: LayerNorm(dropout(x + bias) + input_tensor), the dropout given as a mask."""
    import torch
    tx, tr, tg, tb = _t(x), _t(res), _t(gamma), _t(beta)
    tbias = _t(bias) if bias is not None else None
    u = tx + tbias if tbias is not None else tx
    if keep is not None:
        u = u * torch.from_numpy(keep.astype(np.float32)) * _scale(p)
    y = torch.nn.functional.layer_norm(u + tr, (tx.shape[-1],), tg, tb, eps)
    y.backward(_t(dy, False))
    return dict(y=y.detach().numpy(), dx=tx.grad.numpy(), dres=tr.grad.numpy(), dgamma=tg.grad.numpy(), dbeta=tb.grad.numpy(),
                dbias=tbias.grad.numpy() if tbias is not None else None)


def torch_gelu(t):
    """transformers 2.3.0 modeling_bert.gelu."""
    import torch
    return t * 0.5 * (1.0 + torch.erf(t / math.sqrt(2.0)))


def gelu_eager_fp32(x, bias, dy):
    tx, tb = _t(x), _t(bias)
    y = torch_gelu(tx + tb)
    y.backward(_t(dy, False))
    return dict(y=y.detach().numpy(), dx=tx.grad.numpy(), dbias=tb.grad.numpy())


def distances(got, want, names):
    return {n: float(np.abs(np.asarray(got[n], np.float64) - want[n]).max()) for n in names if want[n] is not None}


# ------------------------------------------------------------------------------------------------------------------ inputs
def tail_inputs(tag, n_rows, H, seed=53, bias=True):
    """x, bias, res, gamma, beta, dy of a seeded case: no exact zeros in x + bias (a kept element is never 0)."""
    x = det_normal(seed, tag + ".x", (n_rows, H), 1.0)
    b = det_normal(seed, tag + ".b", (H,), 0.1) if bias else None
    u = x + b if bias else x
    x = np.where(u == 0, np.float32(0.5), x).astype(np.float32)
    return (x, b, det_normal(seed, tag + ".r", (n_rows, H), 1.0), 1.0 + det_normal(seed, tag + ".g", (H,), 0.1),
            det_normal(seed, tag + ".be", (H,), 0.1), det_normal(seed, tag + ".dy", (n_rows, H), 0.1))


def gelu_inputs(tag, n_rows, N, seed=59):
    return det_normal(seed, tag + ".x", (n_rows, N), 1.5), det_normal(seed, tag + ".b", (N,), 0.1), det_normal(seed, tag + ".dy", (n_rows, N), 0.1)


def layer_weights(hidden, inter, seed=67, ln_jitter=0.1):
    """One layer's parameters under transformers' names, from the fixture's generator (oracle.encoder_ref.det_normal; the scales of
    det_state_dict: weights 0.02, biases and LayerNorm offsets ln_jitter)."""
    sd = {}
    for name, shape in (("attention.self.query", (hidden, hidden)), ("attention.self.key", (hidden, hidden)),
                        ("attention.self.value", (hidden, hidden)), ("attention.output.dense", (hidden, hidden)),
                        ("intermediate.dense", (inter, hidden)), ("output.dense", (hidden, inter))):
        sd[name + ".weight"] = det_normal(seed, name + ".weight", shape, 0.02)
        sd[name + ".bias"] = det_normal(seed, name + ".bias", shape[:1], ln_jitter)
    for name in ("attention.output.LayerNorm", "output.LayerNorm"):
        sd[name + ".weight"] = (1.0 + det_normal(seed, name + ".weight", (hidden,), ln_jitter)).astype(np.float32)
        sd[name + ".bias"] = det_normal(seed, name + ".bias", (hidden,), ln_jitter)
    return sd


# ------------------------------------------------------------------------------------------------------------------ a whole layer
def layer_fp64(hs, lens, sd, n_heads, eps, dout, keeps=None, p_attn=0.0, p_hidden=0.0):
    """ance_amd.layers.BertLayer in fp64.  hs, dout [B, L, H] (dout is zeroed at pad rows here); keeps = (attention keep
    [B, nh, L, L], keep of the first tail [B * L, H], keep of the second) or None.  Returns dict(out, dhs, <parameter name>: grad)."""
    B, L, H = hs.shape
    W = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    rows = A._valid(lens, L)
    hs2 = np.asarray(hs, np.float64).reshape(B * L, H)
    dout = np.where(rows[:, :, None], np.asarray(dout, np.float64), 0.0).reshape(B * L, H)
    ka, k1, k2 = keeps if keeps is not None else (None, None, None)

    def lin(x, name):
        return x @ W[name + ".weight"].T + W[name + ".bias"]

    q, k, v = (lin(hs2, "attention.self." + n).reshape(B, L, H) for n in ("query", "key", "value"))
    ctx = A.attention_fp64(q, k, v, np.zeros_like(q), lens, n_heads, ka, p_attn)["ctx"].reshape(B * L, H)
    x1 = ctx @ W["attention.output.dense.weight"].T
    ln1, ln2 = "attention.output.LayerNorm", "output.LayerNorm"
    zero = np.zeros_like(x1)
    t1 = tail_fp64(x1, W["attention.output.dense.bias"], hs2, W[ln1 + ".weight"], W[ln1 + ".bias"], eps, zero, k1, p_hidden)
    h = t1["y"]
    t0 = h @ W["intermediate.dense.weight"].T
    t = gelu_fp64(t0, W["intermediate.dense.bias"], np.zeros_like(t0))["y"]
    x2 = t @ W["output.dense.weight"].T
    # backward
    b2 = tail_fp64(x2, W["output.dense.bias"], h, W[ln2 + ".weight"], W[ln2 + ".bias"], eps, dout, k2, p_hidden)
    g = {ln2 + ".weight": b2["dgamma"], ln2 + ".bias": b2["dbeta"], "output.dense.bias": b2["dbias"],
         "output.dense.weight": b2["dx"].T @ t}
    bg = gelu_fp64(t0, W["intermediate.dense.bias"], b2["dx"] @ W["output.dense.weight"])
    g["intermediate.dense.bias"], g["intermediate.dense.weight"] = bg["dbias"], bg["dx"].T @ h
    dh = b2["dres"] + bg["dx"] @ W["intermediate.dense.weight"]
    b1 = tail_fp64(x1, W["attention.output.dense.bias"], hs2, W[ln1 + ".weight"], W[ln1 + ".bias"], eps, dh, k1, p_hidden)
    g.update({ln1 + ".weight": b1["dgamma"], ln1 + ".bias": b1["dbeta"], "attention.output.dense.bias": b1["dbias"],
              "attention.output.dense.weight": b1["dx"].T @ ctx})
    dctx = (b1["dx"] @ W["attention.output.dense.weight"]).reshape(B, L, H)
    ba = A.attention_fp64(q, k, v, dctx, lens, n_heads, ka, p_attn)
    dhs = b1["dres"].copy()
    for n, d in (("query", ba["dq"]), ("key", ba["dk"]), ("value", ba["dv"])):
        d = d.reshape(B * L, H)
        g["attention.self.%s.weight" % n], g["attention.self.%s.bias" % n] = d.T @ hs2, d.sum(0)
        dhs += d @ W["attention.self.%s.weight" % n]
    return dict(g, out=b2["y"].reshape(B, L, H), dhs=dhs.reshape(B, L, H))


def layer_torch_forward(ths, rows, W, n_heads, eps, keeps=None, p_attn=0.0, p_hidden=0.0, taps=None):
    """layer_torch's forward on torch tensors, for chaining: ths [B, L, H], rows bool [B, L], W {parameter name: tensor}, keeps three
    tensors of ths's dtype or None.  Returns out [B, L, H] in the graph.  taps: a list that receives (name, tensor) for the
    activations ance_amd.layers.BertLayer(precision="half") holds in 16 bits, each with its gradient retained."""
    import torch
    F = torch.nn.functional
    dt = ths.dtype
    B, L, H = ths.shape
    ka, k1, k2 = keeps if keeps is not None else (None, None, None)

    def tap(name, t):
        if taps is not None:
            t.retain_grad()
            taps.append((name, t))
        return t

    def heads(x):
        return x.view(B, L, n_heads, 64).permute(0, 2, 1, 3)

    def tail(x, dense, ln, res, keep):
        u = x + W[dense + ".bias"]
        if keep is not None:
            u = u * keep.view(B, L, H) * _scale(p_hidden)
        return F.layer_norm(u + res, (H,), W[ln + ".weight"], W[ln + ".bias"], eps)

    q, k, v = (tap(n, F.linear(ths, W["attention.self.%s.weight" % n], W["attention.self.%s.bias" % n])) for n in ("query", "key", "value"))
    mask = ((1.0 - rows.to(dt)) * -10000.0)[:, None, None, :]
    probs = torch.softmax(torch.matmul(heads(q), heads(k).transpose(-1, -2)) / math.sqrt(64) + mask, dim=-1)
    if ka is not None:
        probs = probs * ka * _scale(p_attn)
    ctx = torch.matmul(probs, heads(v)).permute(0, 2, 1, 3).contiguous().view(B, L, H) * rows[:, :, None].to(dt)  # pad rows: zeros
    ctx = tap("ctx", ctx)
    h = tail(tap("attention.output.dense", F.linear(ctx, W["attention.output.dense.weight"])), "attention.output.dense",
             "attention.output.LayerNorm", ths, k1)
    t = tap("gelu", torch_gelu(tap("intermediate.dense", F.linear(h, W["intermediate.dense.weight"])) + W["intermediate.dense.bias"]))
    return tail(tap("output.dense", F.linear(t, W["output.dense.weight"])), "output.dense", "output.LayerNorm", h, k2)


def layer_torch(hs, lens, sd, n_heads, eps, dout, keeps=None, p_attn=0.0, p_hidden=0.0, dtype="float32"):
    """The same layer as transformers' eager expressions in torch on the CPU (fp32: the reference of the bound; float64: a check of
    layer_fp64's hand-written backward), gradients by autograd.  Same dict as layer_fp64."""
    import torch
    dt = getattr(torch, dtype)
    B, L, H = hs.shape
    rows = torch.from_numpy(A._valid(lens, L))
    W = {k: torch.from_numpy(np.array(v)).to(dt).requires_grad_(True) for k, v in sd.items()}
    ths = torch.from_numpy(np.array(hs)).to(dt).requires_grad_(True)
    keeps = None if keeps is None else tuple(None if m is None else torch.from_numpy(m).to(dt) for m in keeps)
    out = layer_torch_forward(ths, rows, W, n_heads, eps, keeps, p_attn, p_hidden)
    out.backward(torch.from_numpy(np.array(dout)).to(dt) * rows[:, :, None].to(dt))
    res = {k_: w.grad.numpy() for k_, w in W.items()}
    res.update(out=out.detach().numpy(), dhs=ths.grad.numpy())
    return res


# ------------------------------------------------------------------------------------------------------------------ the fixture
GOLDEN_FILES = {"rdot": "layer_tail.npz", "bert": "layer_tail_bert.npz"}
TAILS = ("attention.output", "output")


def seam_names(seam):
    return ("y", "dx", "dgamma", "dbeta", "dbias") if seam in TAILS else ("y", "dx", "dbias")


def load_golden(golden_dir, case):
    """(meta of the case, {seam: dict of its committed fp32 arrays}); the `output` tail's res is the `attention.output` tail's y."""
    import json
    import os
    with open(os.path.join(golden_dir, "layer_tail.json")) as f:
        meta = json.load(f)
    g = np.load(os.path.join(golden_dir, meta["files"][case]))
    seams = {s: {k[len(s) + 1:]: g[k] for k in g.files if k.startswith(s + ".") and (s != "output" or not k.startswith("attention."))} for s in SEAMS}
    seams["output"]["res"] = seams["attention.output"]["y"]
    return meta[case], seams


def golden_fp64(seam, t, eps):
    """The fp64 restatement of a seam on its committed fp32 inputs."""
    if seam in TAILS:
        return tail_fp64(t["x"], t["bias"], t["res"], t["gamma"], t["beta"], eps, t["dy"])
    return gelu_fp64(t["x"], t["bias"], t["dy"])
