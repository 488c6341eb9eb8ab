"""The trainable embeddings (ance_amd/embeddings.py -> csrc/embed_train.hip) restated for their tests:

  positions          the position rule of include/ance_amd.h in NumPy ("absolute": the column; "roberta": padding_idx + the running
                     count of non-pad ids, padding_idx at pads -- transformers' create_position_ids_from_input_ids)
  embed_fp64         fp64 NumPy, forward and every gradient given dy, the dropout as an explicit keep mask.  The word table's gradient
                     is returned for the rows that occur only (word_rows, dword [len(word_rows), H]): every other row is zero
  embed_eager_fp32   the eager torch fp32 expression on the CPU with the same mask -- F.embedding x 3, (word + type) + position,
                     F.layer_norm, the mask multiply -- and its autograd gradients: the reference whose own distance from fp64
                     sets the tests' bound (attention_train_util.bound)
  embed_torch_forward   its forward on torch tensors, in the graph: what tests/train_step_util.py chains into a tower
  keep mask          layer_tail_util.tail_keep_mask: the embeddings draw under the layer tail's counter contract
  embed_inputs       seeded tables, LayerNorm parameters and dy
Ids are taken as the kernels take them: clamped into their table first.
"""
import numpy as np

import layer_tail_util as T
from oracle.encoder_ref import det_normal

bound = T.bound
tail_keep_mask = T.tail_keep_mask
NAMES = ("y", "dword", "dpos", "dtype", "dgamma", "dbeta")
GOLDEN_CASES = T.GOLDEN_CASES
GOLDEN_FILES = {"rdot": "embeddings.npz", "bert": "embeddings_bert.npz"}
PARAMS = ("word_embeddings.weight", "position_embeddings.weight", "token_type_embeddings.weight", "LayerNorm.weight", "LayerNorm.bias")
GRAD_OF = dict(zip(PARAMS, ("dword", "dpos", "dtype", "dgamma", "dbeta")))


def _scale(p):
    return 1.0 / (1.0 - float(np.float32(p)))


def clamp_ids(ids, n):
    return np.clip(np.asarray(ids, np.int64), 0, n - 1)


def positions(ids, mode, pad, vocab=None, max_pos=None):
    """[B, L] int64 positions of (clamped) ids."""
    ids = np.asarray(ids, np.int64)
    if vocab is not None:
        ids = clamp_ids(ids, vocab)
    if mode == "absolute":
        p = np.broadcast_to(np.arange(ids.shape[1], dtype=np.int64)[None, :], ids.shape).copy()
    else:
        m = ids != pad
        p = np.cumsum(m, axis=1) * m + pad
    return clamp_ids(p, max_pos) if max_pos is not None else p


def _scatter(keys, g, n, pad=None):
    out = np.zeros((n, g.shape[1]), np.float64)
    np.add.at(out, keys, g)
    if pad is not None and pad >= 0:
        out[pad] = 0.0
    return out


def embed_fp64(ids, types, word, pos, typ, gamma, beta, eps, dy, mode="absolute", pad=None, keep=None, p=0.0):
    """ids, types [B, L] (types None: zeros); dy [B * L, H]; keep bool [B * L, H] or None.  dict(y [B * L, H], word_rows, dword (those
    rows), dpos [max_pos, H], dtype [n_types, H], dgamma, dbeta, positions [B, L])."""
    H = word.shape[1]
    idc = clamp_ids(ids, word.shape[0]).reshape(-1)
    ttc = clamp_ids(types, typ.shape[0]).reshape(-1) if types is not None else np.zeros(idc.shape, np.int64)
    pp = positions(ids, mode, pad, word.shape[0], pos.shape[0])
    pc = pp.reshape(-1)
    v = (word[idc].astype(np.float64) + typ[ttc].astype(np.float64)) + pos[pc].astype(np.float64)
    gamma, beta, dy = (np.asarray(t, np.float64) for t in (gamma, beta, dy))
    mean = v.mean(-1, keepdims=True)
    var = ((v - mean) ** 2).sum(-1, keepdims=True) / H
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (v - mean) * rstd
    k = keep * _scale(p) if keep is not None else 1.0
    y = (xhat * gamma + beta) * k
    d = dy * k
    g = d * gamma
    dv = rstd * (g - g.mean(-1, keepdims=True) - xhat * (g * xhat).mean(-1, keepdims=True))
    rows, inv = np.unique(idc, return_inverse=True)
    dword = np.zeros((len(rows), H), np.float64)
    np.add.at(dword, inv.reshape(-1), dv)
    if pad is not None and pad >= 0:
        dword[rows == pad] = 0.0
    return dict(y=y, word_rows=rows, dword=dword, dpos=_scatter(pc, dv, pos.shape[0], pad if mode == "roberta" else None),
                dtype=_scatter(ttc, dv, typ.shape[0]), dgamma=(d * xhat).sum(0), dbeta=d.sum(0), positions=pp)


def embed_torch_forward(ids, types, tw, tp, tt, tg, tb, eps, mode="absolute", pad=None, keep=None, p=0.0):
    """embed_eager_fp32's forward on torch tensors, for chaining: ids, types NumPy [B, L] (types None: zeros), the five parameters
    tensors, keep a tensor of their dtype shaped like y, or None.  Returns y [B, L, H] in the graph."""
    import torch
    F = torch.nn.functional
    idc = torch.from_numpy(clamp_ids(ids, tw.shape[0])).to(tw.device)
    ttc = torch.from_numpy(clamp_ids(types, tt.shape[0])).to(tw.device) if types is not None else torch.zeros_like(idc)
    pc = torch.from_numpy(positions(ids, mode, pad, tw.shape[0], tp.shape[0])).to(tw.device)
    pad_w = pad if pad is not None and pad >= 0 else None
    e = F.embedding(idc, tw, padding_idx=pad_w) + F.embedding(ttc, tt)
    e = e + F.embedding(pc, tp, padding_idx=pad_w if mode == "roberta" else None)
    y = F.layer_norm(e, (tw.shape[1],), tg, tb, eps)
    if keep is not None:
        y = y * keep.reshape(tuple(y.shape)) * _scale(p)
    return y


def embed_eager_fp32(ids, types, word, pos, typ, gamma, beta, eps, dy, mode="absolute", pad=None, keep=None, p=0.0, dtype="float32",
                     backward=True):
    """transformers' eager BertEmbeddings / RobertaEmbeddings expression in torch on the CPU (dtype float64: a check of embed_fp64's
    hand-written backward), the dropout given as a mask.  Same dict as embed_fp64 (y only with backward=False)."""
    import torch
    dt = getattr(torch, dtype)
    tw, tp, tt, tg, tb = (torch.from_numpy(np.array(t)).to(dt).requires_grad_(backward) for t in (word, pos, typ, gamma, beta))
    y = embed_torch_forward(ids, types, tw, tp, tt, tg, tb, eps, mode, pad, None if keep is None else torch.from_numpy(keep).to(dt), p)
    if not backward:
        return dict(y=y.numpy().reshape(-1, word.shape[1]))
    y.backward(torch.from_numpy(np.array(dy)).to(dt).reshape(y.shape))
    rows = np.unique(clamp_ids(ids, word.shape[0]))
    return dict(y=y.detach().numpy().reshape(-1, word.shape[1]), word_rows=rows, dword=tw.grad.numpy()[rows], dpos=tp.grad.numpy(),
                dtype=tt.grad.numpy(), dgamma=tg.grad.numpy(), dbeta=tb.grad.numpy())


def distances(got, want, names=NAMES):
    return {n: float(np.abs(np.asarray(got[n], np.float64) - want[n]).max()) for n in names}


# ------------------------------------------------------------------------------------------------------------------ inputs
def embed_inputs(tag, H, vocab=1000, max_pos=514, n_types=2, seed=61, std=0.5):
    """word, pos, typ, gamma, beta of a seeded case (std 0.5: sums of three are O(1), like the layer tail's rows)."""
    return (det_normal(seed, tag + ".word", (vocab, H), std), det_normal(seed, tag + ".pos", (max_pos, H), std),
            det_normal(seed, tag + ".type", (n_types, H), std), (1.0 + det_normal(seed, tag + ".g", (H,), 0.1)).astype(np.float32),
            det_normal(seed, tag + ".be", (H,), 0.1))


def embed_dy(tag, n_rows, H, seed=61):
    return det_normal(seed, tag + ".dy", (n_rows, H), 0.1)


def seeded_ids(tag, shape, lo, hi, seed=61):
    """int64 ids in [lo, hi), a deterministic function of the tag."""
    u = det_normal(seed, tag + ".ids", shape, 1.0).view(np.uint32).astype(np.int64)
    return lo + u % (hi - lo)


# ------------------------------------------------------------------------------------------------------------------ the fixture
def load_golden(golden_dir, case):
    """(meta of the case, dict of its committed arrays)."""
    import json
    import os
    with open(os.path.join(golden_dir, "embeddings.json")) as f:
        meta = json.load(f)
    g = np.load(os.path.join(golden_dir, meta["files"][case]))
    return meta[case], {k: g[k] for k in g.files}


def golden_tables(m):
    """The case's five embedding parameters from oracle.encoder_ref.det_state_dict by seed: word, pos, typ, gamma, beta (fp32 NumPy)."""
    from oracle import encoder_ref
    kw = dict(kind="bert", vocab=30522, max_pos=512, prefixes=("",)) if m["kind"] == "bert" else {}
    sd = encoder_ref.det_state_dict(seed=m["seed"], n_layers=0, head=False, ln_jitter=m["ln_jitter"], **kw)
    e = ("" if m["kind"] == "bert" else "roberta.") + "embeddings."
    assert encoder_ref.state_dict_sha256(sd) == m["embeddings_sha256"], "the generator's weights are not these"
    return tuple(sd[e + n].numpy() for n in PARAMS)
