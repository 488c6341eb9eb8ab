"""A whole training step of the trainers' tower, restated for tests/test_train_step.py (the oracle's self-check, CPU) and
tests/test_gpu_train_step.py (the fused pieces composed on the GPU).  Nothing here imports the GPU library at module level.

The tower, stated once and built three ways from one state dict (transformers' parameter names, so that
ance_amd.embeddings.BertEmbeddings / ance_amd.layers.BertLayer load them strict=True):

    embeddings -> N x encoder.layer.i -> h[:, 0] -> embeddingHead (nn.Linear(H, H)) -> norm (nn.LayerNorm(H), eps 1e-5)

  tower_fp64 / tower_eager_fp32   torch on the CPU with autograd, float64 and float32: embeddings_util.embed_torch_forward, N x
                       layer_tail_util.layer_torch_forward, the head.  Every dropout is an explicit keep mask; pad rows of the
                       attention context are zeros, as BertLayer documents.  The fp32 one's distance from the fp64 one is the
                       ref_err of every bound (attention_train_util.bound: 4 x ref_err, floor 16 ulp32)
  device_tower         the same tower from BertEmbeddings and BertLayer on the GPU (imported inside the function)
  step_masks           the keep masks of ONE tower call in draw order -- embeddings, then per layer attention, first tail, second
                       tail: 1 + 3 N consecutive offsets of the one dropout stream; the calls of a step take consecutive blocks
  reference_step       the loss (triplet NLL or in-batch NLL) of a step's tower calls and every parameter gradient
  lamb_update_fp64 / adamw_update_fp64   lamb_util.step_fp64 / adamw_util.step_fp64 behind objective_util.clip_fp64 over a
                       dict of named tensors: the update link's oracle, applied to the device's own gradients
"""
import numpy as np

import adamw_util as W_
import attention_train_util as A
import embeddings_util as E
import lamb_util as U
import layer_tail_util as T
import objective_util as O
from oracle.encoder_ref import det_normal

HEAD_EPS = 1e-5           # nn.LayerNorm's default: the reference's self.norm
VOCAB, MAX_POS = 1000, 514
PLANTED = (7, 77, 777)    # ids that occur in every call of a step; 77 twice in one sequence, 777 as a first token
BASE = dict(H=768, heads=12, inter=3072, N=2, mode="absolute", n_types=2, eps=1e-5, pad=0)
LARGE = dict(H=1024, heads=16, inter=4096, N=1, mode="roberta", n_types=1, eps=1e-12, pad=1)
# No call has a multiple of 16 rows (the tails' workgroups own 16), the three differ (36, 120, 123), and the lengths include 1, 17, 33.
SHAPES = (("query", 12, (12, 5, 1)), ("positive", 40, (40, 17, 33)), ("negative", 41, (33, 41, 9)))
SEED = 0x5EED0123456789AB   # of the dropout stream
# The embeddings are LayerNorm outputs of 768 / 1024 columns: the logits are in the hundreds and the objectives saturated, so a
# triplet whose positive leads (a query whose positive wins) sends a gradient of e^-lead: a rounded zero into its three sequences.
# These seeds of the batches are the first, per step, at which in the reference (tower_state's parameters, dropout off and 0.1)
# every triplet's negative leads by more than 20 / every query's positive trails by more than 8: every sequence of every call
# carries a full gradient.  tests/test_train_step.py asserts it.
TRIPLET_SEEDS, INBATCH_SEEDS = (87, 147, 130), (340, 79)
EMB = tuple("embeddings." + n for n in E.PARAMS)
HEAD = ("embeddingHead.weight", "embeddingHead.bias", "norm.weight", "norm.bias")
WORD = EMB[0]


def layer_prefix(i):
    return "encoder.layer.%d." % i


def param_names(cfg):
    return EMB + tuple(layer_prefix(i) + n for i in range(cfg["N"]) for n in T.LAYER_PARAMS) + HEAD


def group_of(name):
    """lamb_util.GROUPS: 0 (no weight decay) the biases and every LayerNorm, 1 the matrices and the tables."""
    return 0 if name.endswith(".bias") or "LayerNorm" in name or name.startswith("norm.") else 1


# ------------------------------------------------------------------------------------------------------------------ inputs
def tower_state(cfg, seed=73, ln_jitter=0.1):
    """{name: fp32 NumPy}: the word table with std 0.5 as embed_inputs, the layers from layer_weights, the head's LayerNorm with the
    same ln_jitter."""
    H = cfg["H"]
    sd = dict(zip(EMB, E.embed_inputs("tower", H, VOCAB, MAX_POS, cfg["n_types"], seed)))
    for i in range(cfg["N"]):
        sd.update({layer_prefix(i) + k: v for k, v in T.layer_weights(H, cfg["inter"], seed + 1 + i, ln_jitter).items()})
    sd["embeddingHead.weight"] = det_normal(seed, "embeddingHead.weight", (H, H), 0.02)
    sd["embeddingHead.bias"] = det_normal(seed, "embeddingHead.bias", (H,), ln_jitter)
    sd["norm.weight"] = (1.0 + det_normal(seed, "norm.weight", (H,), ln_jitter)).astype(np.float32)
    sd["norm.bias"] = det_normal(seed, "norm.bias", (H,), ln_jitter)
    assert sorted(sd) == sorted(param_names(cfg))
    return sd


def batches(cfg, step=0, seed=79):
    """The three batches of a step -- dict(name, ids [3, L] int64, types or None, lens int32) -- right-padded with the pad id (every
    batch has pads), no pad id inside a sequence, PLANTED in every batch."""
    out = []
    for name, L, lens in SHAPES:
        tag = "step%d.%s" % (step, name)
        ids = E.seeded_ids(tag, (len(lens), L), cfg["pad"] + 1, VOCAB, seed)
        ids[0, 1] = ids[0, 3] = PLANTED[1]
        ids[0, 2] = ids[1, 4] = PLANTED[0]
        ids[1, 0] = PLANTED[2]
        ids[np.arange(L)[None, :] >= np.asarray(lens)[:, None]] = cfg["pad"]
        types = E.seeded_ids(tag + ".tt", ids.shape, 0, 2, seed) if cfg["n_types"] == 2 else None
        out.append(dict(name=name, ids=ids, types=types, lens=np.asarray(lens, np.int32)))
    return out


def inbatch_calls(three, pad):
    """The in-batch form of a step: the query call and ONE context call of six sequences, positives at 0, 1, 2 (the positive batch
    padded to the negative's length)."""
    q, a, b = three
    L = max(a["ids"].shape[1], b["ids"].shape[1])

    def wide(x, fill):
        return None if x is None else np.concatenate([np.pad(t, ((0, 0), (0, L - t.shape[1])), constant_values=fill) for t in x])

    ctx = dict(name="contexts", ids=wide((a["ids"], b["ids"]), pad), lens=np.concatenate([a["lens"], b["lens"]]),
               types=None if a["types"] is None else wide((a["types"], b["types"]), 0))
    return [q, ctx]


def step_calls(cfg, kind, step):
    """The tower calls of step `step`: three for the triplet objective, two for the in-batch one."""
    if kind == "triplet":
        return batches(cfg, step, TRIPLET_SEEDS[step])
    return inbatch_calls(batches(cfg, step, INBATCH_SEEDS[step]), cfg["pad"])


def occurring_rows(calls, pad):
    """The word rows that get a gradient in a step: the ids of every call, without the pad id."""
    rows = np.unique(np.concatenate([c["ids"].reshape(-1) for c in calls]))
    return rows[rows != pad]


# ------------------------------------------------------------------------------------------------------------------ the masks
def draws_per_call(cfg):
    return 1 + 3 * cfg["N"]


def step_masks(p, seed, first_offset, cfg, lens, L):
    """The keep masks of one tower call in draw order, from offset first_offset on: dict(embeddings=[B * L, H], layers=[(attention
    [B, heads, L, L], first tail [B * L, H], second tail [B * L, H])] * N)."""
    B, H, off = len(lens), cfg["H"], first_offset
    emb = E.tail_keep_mask(p, seed, off, B * L, H)
    layers = []
    for _ in range(cfg["N"]):
        layers.append((A.keep_masks(p, seed, off + 1, lens, cfg["heads"], L), T.tail_keep_mask(p, seed, off + 2, B * L, H),
                       T.tail_keep_mask(p, seed, off + 3, B * L, H)))
        off += 3
    return dict(embeddings=emb, layers=layers)


def calls_masks(p, seed, first_offset, cfg, calls):
    """step_masks of every call of a step: consecutive blocks of 1 + 3 N offsets.  None without dropout."""
    if not p > 0:
        return [None] * len(calls)
    return [step_masks(p, seed, first_offset + k * draws_per_call(cfg), cfg, c["lens"], c["ids"].shape[1]) for k, c in enumerate(calls)]


# ------------------------------------------------------------------------------------------------------------------ the tower in torch
def tower_forward(W, call, cfg, masks=None, p=0.0, taps=None):
    """One tower call on torch tensors W {name: tensor}: [B, H] in the graph."""
    import torch
    F = torch.nn.functional
    dt = W[WORD].dtype
    B, L = call["ids"].shape

    def t(m):
        return torch.from_numpy(m).to(dt)

    h = E.embed_torch_forward(call["ids"], call["types"], *(W[n] for n in EMB), cfg["eps"], cfg["mode"], cfg["pad"],
                              None if masks is None else t(masks["embeddings"]), p)
    rows = torch.from_numpy(A._valid(call["lens"], L))
    for i in range(cfg["N"]):
        pre = layer_prefix(i)
        keeps = None if masks is None else tuple(t(m) for m in masks["layers"][i])
        named = None if taps is None else []
        h = T.layer_torch_forward(h, rows, {n: W[pre + n] for n in T.LAYER_PARAMS}, cfg["heads"], cfg["eps"], keeps, p, p, named)
        if taps is not None:
            taps.extend(("%s.%s%s" % (call["name"], pre, n), x) for n, x in named)
    e = F.linear(h[:, 0].contiguous(), W["embeddingHead.weight"], W["embeddingHead.bias"])
    return F.layer_norm(e, (cfg["H"],), W["norm.weight"], W["norm.bias"], HEAD_EPS)


def loss_torch(kind, embs):
    """triplet: ance_amd.loss.nll_loss's mean of -log_softmax([q.a, q.b])[0]; inbatch: biencoder_nll_loss's mean of
    -log_softmax(q ctx^T)[i, i] (positives at 0, 1, 2)."""
    import torch
    if kind == "triplet":
        q, a, b = embs
        return -torch.log_softmax(torch.stack([(q * a).sum(-1), (q * b).sum(-1)], 1), 1)[:, 0].mean()
    q, c = embs
    return -torch.log_softmax(q @ c.t(), 1)[torch.arange(len(q)), torch.arange(len(q))].mean()


def reference_step(sd, calls, cfg, kind, masks=None, p=0.0, dtype="float64", taps=None, loss_scale=1.0):
    """dict(loss, embs [np], grads {name: np}) of one step's tower calls and one backward in torch on the CPU."""
    import torch
    dt = getattr(torch, dtype)
    W = {k: torch.from_numpy(np.array(v)).to(dt).requires_grad_(True) for k, v in sd.items()}
    masks = masks if masks is not None else [None] * len(calls)
    embs = [tower_forward(W, c, cfg, m, p, taps) for c, m in zip(calls, masks)]
    loss = loss_torch(kind, embs)
    (loss * loss_scale).backward()
    return dict(loss=float(loss.detach()), embs=[e.detach().numpy() for e in embs], grads={k: w.grad.numpy() for k, w in W.items()})


def tower_fp64(sd, calls, cfg, kind, masks=None, p=0.0, **kw):
    return reference_step(sd, calls, cfg, kind, masks, p, "float64", **kw)


def tower_eager_fp32(sd, calls, cfg, kind, masks=None, p=0.0, **kw):
    return reference_step(sd, calls, cfg, kind, masks, p, "float32", **kw)


# ------------------------------------------------------------------------------------------------------------------ the tower on the GPU
def device_tower(cfg, sd, p, precision="fp32", device="cuda:0"):
    """The tower from the library's modules, loaded strict=True from sd."""
    import torch

    from ance_amd.embeddings import BertEmbeddings
    from ance_amd.layers import BertLayer
    nn = torch.nn

    class Encoder(nn.Module):
        def __init__(self):
            super().__init__()
            self.layer = nn.ModuleList([BertLayer(cfg["H"], cfg["heads"], cfg["inter"], cfg["eps"], p, p, precision=precision)
                                        for _ in range(cfg["N"])])

    class Tower(nn.Module):
        def __init__(self):
            super().__init__()
            self.embeddings = BertEmbeddings(VOCAB, cfg["H"], MAX_POS, cfg["n_types"], cfg["eps"], p, cfg["pad"], cfg["mode"])
            self.encoder = Encoder()
            self.embeddingHead = nn.Linear(cfg["H"], cfg["H"])
            self.norm = nn.LayerNorm(cfg["H"], eps=HEAD_EPS)

        def forward(self, ids, types, lens):
            h = self.embeddings(ids, types)
            layers = self.encoder.layer
            if precision == "half":   # chained through the 16-bit copy: one activation cast in the whole tower
                h16 = None
                for layer in layers[:-1]:
                    h, h16 = layer(h, lens, hidden_states_half=h16, return_half=True)
                h = layers[-1](h, lens, hidden_states_half=h16)
            else:
                for layer in layers:
                    h = layer(h, lens)
            return self.norm(self.embeddingHead(h[:, 0].contiguous()))

    tower = Tower().to(device)
    tower.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v, np.float32)) for k, v in sd.items()}, strict=True)
    assert tuple(n for n, _ in tower.named_parameters()) == param_names(cfg)   # transformers' names, in module order
    return tower


def param_groups(tower):
    """The two groups of lamb_util.GROUPS over the tower's named parameters."""
    named = list(tower.named_parameters())
    return [dict(params=[q for n, q in named if group_of(n) == k], lr=U.GROUPS[k]["lr"], weight_decay=U.GROUPS[k]["weight_decay"])
            for k in range(len(U.GROUPS))]


# ------------------------------------------------------------------------------------------------------------------ the update link
def lamb_update_fp64(params, grads, moments, max_norm=1.0):
    """(total norm, coef, {name: (p, m, v, wn, an, tr)}): objective_util.clip_fp64 over every gradient, then lamb_util.step_fp64 per
    tensor with its group's hyper-parameters.  moments {name: (m, v)}; a missing name starts from zeros."""
    total, coef = O.clip_fp64(list(grads.values()), max_norm)
    out = {}
    for n, g in grads.items():
        m, v = moments.get(n) or (np.zeros(g.shape), np.zeros(g.shape))
        gr = U.GROUPS[group_of(n)]
        out[n] = U.step_fp64(params[n], np.asarray(g, np.float64) * coef, m, v, gr["lr"], U.BETAS, U.EPS, gr["weight_decay"], False)
    return total, coef, out


def adamw_update_fp64(params, grads, moments, t, max_norm=1.0):
    """The same with adamw_util.step_fp64; t: the step count after this step.  {name: (p, m, v)}."""
    total, coef = O.clip_fp64(list(grads.values()), max_norm)
    out = {}
    for n, g in grads.items():
        m, v = moments.get(n) or (np.zeros(g.shape), np.zeros(g.shape))
        gr = U.GROUPS[group_of(n)]
        out[n] = W_.step_fp64(params[n], np.asarray(g, np.float64) * coef, m, v, t, gr["lr"], U.BETAS, U.EPS, gr["weight_decay"])
    return total, coef, out


def adamw_update_fp32(params, grads, moments, t, max_norm=1.0):
    """clip_grad_norm_ and transformers 2.3.0's AdamW.step statement by statement in NumPy fp32: the fp32 reference whose own
    distance from adamw_update_fp64 is the ref_err of adamw_util.bound.  {name: (p, m, v)}."""
    f = np.float32
    total = f(np.sqrt(sum(float(np.dot(g.ravel().astype(np.float64), g.ravel().astype(np.float64))) for g in grads.values())))
    coef = min(f(max_norm) / (total + f(1e-6)), f(1.0))
    b1, b2 = U.BETAS
    out = {}
    for n, g in grads.items():
        m, v = moments.get(n) or (np.zeros(g.shape, f), np.zeros(g.shape, f))
        gr = U.GROUPS[group_of(n)]
        g = np.asarray(g, f) * coef
        m = np.asarray(m, f) * f(b1) + f(1 - b1) * g
        v = np.asarray(v, f) * f(b2) + f(1 - b2) * g * g
        q = np.asarray(params[n], f) + f(-W_.step_size(gr["lr"], U.BETAS, t, True)) * (m / (np.sqrt(v) + f(U.EPS)))
        if gr["weight_decay"] > 0:
            q = q + f(-gr["lr"] * gr["weight_decay"]) * q
        out[n] = (q, m, v)
    return out


# ------------------------------------------------------------------------------------------------------------------ comparing
def compare(tag, got, want, ref_err, names=None, floor_ulps=16.0):
    """Prints name, d, ref_err, ratio, bound per tensor and returns (the tensors beyond max(4 x ref_err, floor_ulps ulp32 of the
    largest |want|), the largest d / bound)."""
    bad, worst = [], 0.0
    for n in (names if names is not None else sorted(want)):
        w = np.asarray(want[n], np.float64)
        d = float(np.abs(np.asarray(got[n], np.float64) - w).max(initial=0.0))
        r = float(ref_err[n])
        b = max(4.0 * r, floor_ulps * A.ulp32(np.abs(w).max(initial=0.0)))
        worst = max(worst, d / b)
        print("%-28s %-58s d %.3e  ref_err %.3e  ratio %7.2f  bound %.3e%s"
              % (tag, n, d, r, d / r if r > 0 else float("nan"), b, "" if d <= b else "  BEYOND ITS BOUND"))
        if not d <= b:
            bad.append((n, d, r, b))
    return bad, worst


def distances(a, b, names=None):
    return {n: float(np.abs(np.asarray(a[n], np.float64) - np.asarray(b[n], np.float64)).max(initial=0.0))
            for n in (names if names is not None else b)}
