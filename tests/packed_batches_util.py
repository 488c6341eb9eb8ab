"""The packed gather (ance_amd.batches.PackedBatches -> csrc/batch_gather_packed.hip) restated in NumPy for tests/test_packed_batches.py
(CPU) and tests/test_gpu_packed_batches.py: batches_util.numpy_gather (the padded gather of a plan) composed with packed_util.pack
(the plan and the packed keys of ance_pack_tokens).  Nothing here imports the GPU library.

  tower_batches   per tower of a form: the padded ids and the lengths (what lens_from_mask makes of the padded mask: the number of
                  mask entries that are set, holes included) of the WHOLE item stream, cut into chunks of chunk_len
  batch_totals    int64 [n_batches, n_towers]: the token count of every batch
  packed_batch    packed_util.pack of one tower's share of one batch at a capacity
  dpr_worst       the DPR forms' bound: the batch totals with every line's negative counted at the line's longest one
"""
import numpy as np

import batches_util as U
import packed_util as P

TOWERS = {True: ("q", "a", "b"), False: ("q", "a")}


def chunk_of(cache, chunk_len):
    L = cache.embedding_size
    return L if chunk_len is None or L <= chunk_len else chunk_len


def tower_batches(form, plan, query_cache, passage_cache, chunk_len=None):
    """{tower: (ids int32 [n_items * C, chunk], lens int64 [n_items * C], C)} of a plan."""
    dpr, out = form.startswith("dpr"), {}
    for name in TOWERS[form.endswith("triplet")]:
        cache = query_cache if name == "q" else passage_cache
        ids, mask, _ = U.numpy_gather(cache, plan[name], dpr, name != "q")
        ch = chunk_of(cache, None if name == "q" else chunk_len)
        C = cache.embedding_size // ch
        out[name] = (ids.reshape(-1, ch), mask.reshape(-1, ch).sum(1).astype(np.int64), C)
    return out


def batch_totals(towers, n_items, B):
    n_batches = -(-n_items // B)
    out = np.zeros((n_batches, len(towers)), np.int64)
    for j, (ids, lens, C) in enumerate(towers.values()):
        for k in range(n_batches):
            out[k, j] = lens[k * B * C:(k + 1) * B * C].sum()
    return out


def packed_batch(tower, first, b, R, mode, pad, vocab, max_pos, missing=0):
    """packed_util.pack of items first .. first + b - 1 of a tower's stream; `missing` further items are empty sequences."""
    ids, lens, C = tower
    ids, lens = ids[first * C:(first + b) * C], lens[first * C:(first + b) * C]
    if missing:
        ids = np.concatenate([ids, np.zeros((missing * C, ids.shape[1]), ids.dtype)])
        lens = np.concatenate([lens, np.zeros(missing * C, lens.dtype)])
    return P.pack(ids, None, lens, R, mode, pad, vocab, max_pos)


def dpr_worst(tb, query_cache, passage_cache):
    """[n_towers] ints from the lines alone: the largest batch total with every line's negative at its longest."""
    ql = (query_cache.ids() != 0).sum(1).astype(np.int64)
    pl = (passage_cache.ids() != 0).sum(1).astype(np.int64)
    worst = np.array([pl[tb._neg[s:s + k]].max() for s, k in zip(tb._neg_start.tolist(), tb._n_neg.tolist())], np.int64)
    q, pos = ql[tb._qid], pl[tb._pos]
    per = [q, pos, worst] if tb.triplet else [np.repeat(q, 2), np.stack([pos, worst], 1).reshape(-1)]
    B = tb.batch_size
    return [max(int(x[k:k + B].sum()) for k in range(0, len(x), B)) for x in per]
