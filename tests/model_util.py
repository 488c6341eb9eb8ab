"""The first-row attention core (ance_amd.attention.attention_first_row -> csrc/attention_row0.hip) and the models of
ance_amd/model.py, restated for tests/test_model.py (CPU) and tests/test_gpu_attention_row0.py / test_gpu_model.py.  Nothing here
imports the GPU library at module level.

  first_row_fp64       the statement of include/ance_amd.h in NumPy (fp64 by default): per sequence and head t_j = 0.125 (q0 . K_j),
                       P = softmax over j < len, P' = keep o P / (1 - p), ctx0 = sum P'_j V_j, and the gradient written out by hand
  first_row_keep       the keep masks of query row 0, restated from the Philox contract (attention_train_util.keep_mask, n_q = 1)
  eager_first_row      transformers' eager expression for a ONE-row query in torch on the CPU, fp32 or -- with a 16-bit dtype -- with
                       autocast's roundings (attention_half_util.eager_half); gradients by autograd.  Its distance from fp64 sets
                       the bounds: attention_train_util.bound for fp32, attention_half_util.bound16 for 16 bits
  first_row_masks      train_step_util.step_masks of a tower whose LAST layer runs on first rows: the attention mask of that layer is
                       the full mask's query row 0 (every other query row dropped: nothing reads them), its two tail masks are those
                       of a B-row call laid at rows b * L of a full-size mask -- so train_step_util.tower_forward, which reads only
                       h[:, 0] of the last layer, is the model's oracle as it stands
"""
import numpy as np

import attention_half_util as HU
import attention_train_util as A
import layer_tail_util as T
import train_step_util as S

NAMES = ("ctx", "dq", "dk", "dv")
SWEEP_BATCHES = ((0, 1, 2, 3, 4), (5, 63, 64, 65, 127), (128, 129, 511, 512))   # the issue's lengths, B <= 5


# ------------------------------------------------------------------------------------------------------------------ the kernel's statement
def first_row_keep(p, seed, offset, lens, n_heads, L):
    """bool [B, n_heads, L]: the keys that query row 0 of (sequence s, head h) keeps under (seed, offset)."""
    return np.stack([np.stack([A.keep_mask(p, seed, offset, s, h, n_heads, 1, L)[0] for h in range(n_heads)]) for s in range(len(lens))])


def first_row_inputs(tag, lens, n_heads, L=None, q_scale=1.0, seed=37, dtype=None):
    """q0, dctx0 [B, H], k, v [B, L, H] fp32 (every row filled, pad rows included), lens; rounded to a 16-bit dtype when given."""
    q, k, v, g, lens = A.seeded_inputs(tag, lens, n_heads, L=L or max(int(max(lens)), 1), q_scale=q_scale, seed=seed)
    out = [np.ascontiguousarray(q[:, 0]), k, v, np.ascontiguousarray(g[:, 0])]
    if dtype is not None:
        out = [HU.round16(x, dtype) for x in out]
    return out + [lens]


def first_row_fp64(q0, k, v, dctx0, lens, n_heads, keep=None, p=0.0, dtype=np.float64):
    """dict(ctx [B, H], dq [B, H], dk [B, L, H], dv [B, L, H]) in `dtype`; a sequence of length 0 gives zeros everywhere."""
    f = dtype
    B, L, H = k.shape
    out = dict(ctx=np.zeros((B, H), f), dq=np.zeros((B, H), f), dk=np.zeros((B, L, H), f), dv=np.zeros((B, L, H), f))
    scale = f(1.0) / (f(1.0) - f(np.float32(p))) if keep is not None else f(1.0)
    for s, n in enumerate(np.asarray(lens)):
        n = int(n)
        if n <= 0:
            continue
        for h in range(n_heads):
            c = slice(A.HEAD * h, A.HEAD * h + A.HEAD)
            q, K, V, g = (np.asarray(x, f) for x in (q0[s, c], k[s, :n, c], v[s, :n, c], dctx0[s, c]))
            t = f(0.125) * (K @ q)
            e = np.exp(t - t.max())
            P = e / e.sum()
            kp = keep[s, h, :n].astype(f) * scale if keep is not None else np.ones(n, f)
            Pd = P * kp
            out["ctx"][s, c] = Pd @ V
            dP = kp * (V @ g)
            dS = P * (dP - (dP * P).sum())
            out["dq"][s, c] = f(0.125) * (dS @ K)
            out["dk"][s, :n, c] = f(0.125) * dS[:, None] * q[None, :]
            out["dv"][s, :n, c] = Pd[:, None] * g[None, :]
    return out


def autograd_first_row(q0, k, v, dctx0, lens, n_heads, keep=None, p=0.0):
    """The same quantities by torch autograd in fp64 through softmax: the check of first_row_fp64's hand-written gradient."""
    import torch
    B, L, H = k.shape
    tq, tk, tv = (torch.from_numpy(np.asarray(x, np.float64)).requires_grad_(True) for x in (q0, k, v))
    ctx = torch.zeros(B, H, dtype=torch.float64)
    rows = []
    for s, n in enumerate(np.asarray(lens)):
        heads = []
        for h in range(n_heads):
            c = slice(A.HEAD * h, A.HEAD * h + A.HEAD)
            if n <= 0:
                heads.append(torch.zeros(A.HEAD, dtype=torch.float64))
                continue
            P = torch.softmax(0.125 * (tk[s, :n, c] @ tq[s, c]), 0)
            if keep is not None:
                P = P * torch.from_numpy(keep[s, h, :n].astype(np.float64)) * (1.0 / (1.0 - float(np.float32(p))))
            heads.append(P @ tv[s, :n, c])
        rows.append(torch.cat(heads))
    ctx = torch.stack(rows)
    ctx.backward(torch.from_numpy(np.asarray(dctx0, np.float64)))
    return dict(ctx=ctx.detach().numpy(), dq=tq.grad.numpy(), dk=tk.grad.numpy(), dv=tv.grad.numpy())


def eager_first_row(q0, k, v, dctx0, lens, n_heads, keep=None, p=0.0, dtype=None):
    """transformers' eager BertSelfAttention expression for a one-row query (matmul, / 8, additive -10000 mask, softmax, dropout as a
    mask, matmul) in torch on the CPU: fp32, or with a 16-bit dtype the roundings of autocast (every matmul's result, the scaled and
    masked scores and the probabilities are rounded to the dtype; softmax runs in fp32).  Pad rows and sequences of length 0 are
    zeroed, as the kernel writes them.  Same dict as first_row_fp64, fp32 arrays."""
    import torch
    B, L, H = k.shape
    lens = np.asarray(lens)
    rows = A._valid(lens, L)
    io = torch.float32 if dtype is None else dtype
    tq, tk, tv = (torch.from_numpy(np.array(x, np.float32)).to(io).requires_grad_(True) for x in (q0, k, v))

    def mm(a, b):
        return a @ b if dtype is None else (a.float() @ b.float()).to(dtype)

    qh = tq.view(B, 1, n_heads, A.HEAD).permute(0, 2, 1, 3)
    kh, vh = (x.view(B, L, n_heads, A.HEAD).permute(0, 2, 1, 3) for x in (tk, tv))
    mask = torch.from_numpy(((1.0 - rows.astype(np.float32)) * -10000.0))[:, None, None, :].to(io)
    scores = mm(qh, kh.transpose(-1, -2)) / 8.0 + mask
    probs = torch.softmax(scores.float(), dim=-1)
    if keep is not None:
        probs = probs * torch.from_numpy(keep.astype(np.float32))[:, :, None, :] * (1.0 / (1.0 - float(np.float32(p))))
    ctx = mm(probs.to(io), vh).permute(0, 2, 1, 3).contiguous().view(B, H)
    some = (lens > 0)[:, None]
    ctx.backward(torch.from_numpy(np.where(some, np.asarray(dctx0, np.float32), np.float32(0))).to(io))
    z = rows[:, :, None]
    return dict(ctx=np.where(some, ctx.detach().float().numpy(), 0), dq=np.where(some, tq.grad.float().numpy(), 0),
                dk=np.where(z, tk.grad.float().numpy(), 0), dv=np.where(z, tv.grad.float().numpy(), 0))


def distances(got, want):
    return {n: float(np.abs(np.asarray(got[n], np.float64) - want[n]).max()) for n in NAMES}


def check(tag, got, want, ref_err, dtype=None):
    """Prints every measured distance, then asserts them all: fp32 within A.bound, 16 bits within HU.bound16."""
    bad = []
    for n in NAMES:
        d = float(np.abs(np.asarray(got[n], np.float64) - want[n]).max())
        big = float(np.abs(want[n]).max())
        b = A.bound(ref_err[n], big) if dtype is None else HU.bound16(ref_err[n], big, dtype)
        print("%-40s %-4s max|delta| %.3e  eager %.3e  ratio %5.2f  bound %.3e" % (tag, n, d, ref_err[n], d / max(ref_err[n], 1e-300), b))
        if not d <= b:
            bad.append((n, d, b))
    assert not bad, (tag, bad)


def reference(tag, lens, n_heads, L=None, q_scale=1.0, p=0.0, seed=0, offset=0, dtype=None):
    """Inputs, the fp64 statement and the eager expression's distances from it for one seeded case."""
    q0, k, v, g, lens = first_row_inputs(tag, lens, n_heads, L, q_scale, dtype=dtype)
    keep = first_row_keep(p, seed, offset, lens, n_heads, k.shape[1]) if p > 0 else None
    want = first_row_fp64(q0, k, v, g, lens, n_heads, keep, p)
    ref = distances(eager_first_row(q0, k, v, g, lens, n_heads, keep, p, dtype), want)
    return (q0, k, v, g, lens), want, ref, keep


# ------------------------------------------------------------------------------------------------------------------ the model's masks
def first_row_masks(p, seed, first_offset, cfg, lens, L):
    """S.step_masks for a tower whose last layer is BertLayer.forward_first_rows.  Layers 0 .. N - 2 and the embeddings are the full
    call's.  Last layer: the attention mask is the full one (the model's row-0 mask IS its query row 0, and tower_forward reads no
    other query row of the last layer); each tail mask is all-kept except rows b * L, which carry row b of the B-ROW call's mask."""
    B, H = len(lens), cfg["H"]
    masks = S.step_masks(p, seed, first_offset, cfg, lens, L)
    off = first_offset + 1 + 3 * (cfg["N"] - 1)
    att = masks["layers"][-1][0]
    tails = []
    for k in (1, 2):
        small = T.tail_keep_mask(p, seed, off + k, B, H)
        full = np.ones((B * L, H), dtype=small.dtype)
        full[np.arange(B) * L] = small
        tails.append(full)
    masks["layers"][-1] = (att, tails[0], tails[1])
    return masks


def calls_first_row_masks(p, seed, first_offset, cfg, calls):
    """first_row_masks of every call of a step: consecutive blocks of 1 + 3 N offsets.  None without dropout."""
    if not p > 0:
        return [None] * len(calls)
    return [first_row_masks(p, seed, first_offset + k * S.draws_per_call(cfg), cfg, c["lens"], c["ids"].shape[1]) for k, c in enumerate(calls)]


def model_state(cfg, seed=73, out_dim=768, prefix="roberta."):
    """S.tower_state under the model's names: the tower below `prefix`, and the head H -> out_dim (the reference's Linear(hidden,
    768) + LayerNorm(768))."""
    from oracle.encoder_ref import det_normal
    sd = S.tower_state(cfg, seed)
    out = {}
    for k, v in sd.items():
        if k.startswith("embeddingHead.") or k.startswith("norm."):
            continue
        out[prefix + k] = v
    out["embeddingHead.weight"] = det_normal(seed, "embeddingHead.weight.%d" % out_dim, (out_dim, cfg["H"]), 0.02)
    out["embeddingHead.bias"] = det_normal(seed, "embeddingHead.bias.%d" % out_dim, (out_dim,), 0.1)
    out["norm.weight"] = (1.0 + det_normal(seed, "norm.weight.%d" % out_dim, (out_dim,), 0.1)).astype(np.float32)
    out["norm.bias"] = det_normal(seed, "norm.bias.%d" % out_dim, (out_dim,), 0.1)
    return out


# ------------------------------------------------------------------------------------------------------------------ the golden step
WHOLE, SAMPLE = 4096, 256   # SAMPLE: what keeps three models' fp64 gradients (99k elements) in one file under 1 MiB


def sample_index(name, n, count=SAMPLE):
    """The flat indices of tests/golden/model_step.npz's sample of a tensor of n > WHOLE elements: a fixed odd stride from an
    offset keyed on the tensor's name (the generator and the tests share this function; nothing random is stored)."""
    import zlib
    start = zlib.crc32(name.encode("utf8")) % n
    return (start + np.arange(count, dtype=np.int64) * (2 * (n // (2 * count + 3)) + 1)) % n


def golden_view(name, grad, word_rows=None):
    """What the fixture keeps of a gradient: for a word table the rows that occur, then the tensor whole when it has at most WHOLE
    elements, otherwise its sample_index elements.  fp64, flat."""
    g = np.asarray(grad, np.float64)
    if word_rows is not None and name.endswith("word_embeddings.weight"):
        g = g[word_rows]
    g = g.reshape(-1)
    return g if g.size <= WHOLE else g[sample_index(name, g.size)]


# ------------------------------------------------------------------------------------------------------------------ the model's oracle
def tower_forward(W, call, cfg, masks=None, p=0.0, prefix="roberta.", head=True):
    """S.tower_forward on a model's state (the tower's names below `prefix`), with the head's width taken from its weights (H -> 768)
    or, head=False, the last layer's first rows themselves (BiEncoder).  With a head of width H and prefix "" it IS
    S.tower_forward (tests/test_model.py holds the two together bit for bit)."""
    import torch
    F = torch.nn.functional
    Wt = {k[len(prefix):]: v for k, v in W.items() if k.startswith(prefix)}
    if not head:
        return _first_rows(Wt, call, cfg, masks, p)
    e = F.linear(_first_rows(Wt, call, cfg, masks, p), W["embeddingHead.weight"], W["embeddingHead.bias"])
    return F.layer_norm(e, (e.shape[-1],), W["norm.weight"], W["norm.bias"], S.HEAD_EPS)


def _first_rows(Wt, call, cfg, masks, p):
    """h[:, 0] of the last layer: the body of S.tower_forward up to its head, statement by statement."""
    import torch

    import embeddings_util as E
    dt = Wt[S.WORD].dtype
    B, L = call["ids"].shape

    def t(m):
        return torch.from_numpy(m).to(dt)

    h = E.embed_torch_forward(call["ids"], call["types"], *(Wt[n] for n in S.EMB), cfg["eps"], cfg["mode"], cfg["pad"],
                              None if masks is None else t(masks["embeddings"]), p)
    rows = torch.from_numpy(A._valid(call["lens"], L))
    for i in range(cfg["N"]):
        pre = S.layer_prefix(i)
        keeps = None if masks is None else tuple(t(m) for m in masks["layers"][i])
        h = T.layer_torch_forward(h, rows, {n: Wt[pre + n] for n in T.LAYER_PARAMS}, cfg["heads"], cfg["eps"], keeps, p, p, None)
    return h[:, 0].contiguous()


def reference_step(sd, prefixes, calls, cfg, kind, masks=None, p=0.0, dtype="float64", head=True):
    """S.reference_step for a model: call k runs the tower below prefixes[k].  dict(loss, embs, grads {name: np})."""
    import torch
    dt = getattr(torch, dtype)
    W = {k: torch.from_numpy(np.array(v)).to(dt).requires_grad_(True) for k, v in sd.items()}
    masks = masks if masks is not None else [None] * len(calls)
    embs = [tower_forward(W, c, cfg, m, p, pre, head) for c, m, pre in zip(calls, masks, prefixes)]
    loss = S.loss_torch(kind, embs)
    loss.backward()
    return dict(loss=float(loss.detach()), embs=[e.detach().numpy() for e in embs],
                grads={k: (w.grad.numpy() if w.grad is not None else np.zeros(w.shape)) for k, w in W.items()})
