"""Packed token rows (ance_amd/packing.py -> csrc/pack_rows.hip) restated for tests/test_packing.py (CPU) and the GPU tests
test_gpu_packing.py / test_gpu_packed_model.py.  Nothing here imports the GPU library at module level.

  plan             the statement of include/ance_amd.h in NumPy: len = clamp(lens, 0, L), off = the exclusive prefix sum, kept iff
                   off + len <= R; seq_off (T for a dropped sequence and for the last entry), seq_kept (-1: dropped), T, dropped
  pack             plan + the packed ids, types and positions of R rows, the slack rows included
  unpack_rows      a packed-row array [R, ..] laid into the padded shape: out[s * L + l] = packed[off_s + l] for l < kept_s, `fill`
                   everywhere else -- the remapper that turns the keep masks of an R-row call into the masks reference_step takes
  packed_masks     model_util.first_row_masks for a tower that runs over R packed rows: the attention masks are the padded call's
                   (the same bits), the embeddings' mask and the tails' masks of every layer but the last are those of an R-ROW call
                   at the packed row index, remapped; the last layer's tails are the B-row call's, as in the padded model
"""
import numpy as np

import embeddings_util as E
import layer_tail_util as T
import model_util as M
import train_step_util as S


def plan(lens, L, R):
    """dict(len, seq_off [n + 1], seq_kept [n], T, dropped)."""
    ln = np.clip(np.asarray(lens, np.int64), 0, L)
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]) if len(ln) else np.zeros(0, np.int64)
    kept = off + ln <= R
    total = int((ln * kept).sum())
    assert not kept.size or not (np.diff(kept.astype(np.int8)) > 0).any()   # the dropped sequences are a suffix
    seq_off = np.concatenate([np.where(kept, off, total), [total]]).astype(np.int32)
    return dict(len=ln, seq_off=seq_off, seq_kept=np.where(kept, ln, -1).astype(np.int32), T=total, dropped=int((~kept).sum()))


def pack(ids, types, lens, R, mode, pad, vocab, max_pos):
    """plan's dict + ids, types (None without types), positions: int32 [R].  The ids travel as they are; the positions are
    embeddings_util.positions of the padded batch, its clamps included."""
    ids = np.asarray(ids, np.int64)
    B, L = ids.shape
    out = plan(lens, L, R)
    pos = E.positions(ids, mode, pad, vocab, max_pos)
    pid = np.full(R, pad if pad is not None and pad >= 0 else 0, np.int32)
    ppos = np.full(R, pad if mode == "roberta" else 0, np.int32)
    ptt = np.zeros(R, np.int32) if types is not None else None
    for s in range(B):
        n, o = int(out["seq_kept"][s]), int(out["seq_off"][s])
        if n > 0:
            pid[o:o + n], ppos[o:o + n] = ids[s, :n], pos[s, :n]
            if types is not None:
                ptt[o:o + n] = np.asarray(types)[s, :n]
    out.update(ids=pid, types=ptt, positions=ppos)
    return out


def unpack_rows(packed, seq_off, seq_kept, L, fill):
    """[R, ..] -> [B * L, ..]: row s * L + l takes packed row seq_off[s] + l for l < seq_kept[s]; every other row is `fill`."""
    packed = np.asarray(packed)
    B = len(seq_kept)
    out = np.full((B * L,) + packed.shape[1:], fill, packed.dtype)
    for s in range(B):
        n, o = int(seq_kept[s]), int(seq_off[s])
        if n > 0:
            out[s * L:s * L + n] = packed[o:o + n]
    return out


def pack_rows(padded, seq_off, seq_kept, L, R, fill=0):
    """The inverse on the covered rows: [B * L, ..] -> [R, ..], slack rows `fill`."""
    padded = np.asarray(padded)
    out = np.full((R,) + padded.shape[1:], fill, padded.dtype)
    for s in range(len(seq_kept)):
        n, o = int(seq_kept[s]), int(seq_off[s])
        if n > 0:
            out[o:o + n] = padded[s * L:s * L + n]
    return out


def packed_masks(p, seed, first_offset, cfg, lens, L, R):
    """model_util.first_row_masks with the row-wise masks of the packed tower: see the module docstring.  Pad rows keep everything
    (nothing that reaches a loss reads them)."""
    pl = plan(lens, L, R)
    H = cfg["H"]
    masks = M.first_row_masks(p, seed, first_offset, cfg, lens, L)

    def remapped(offset):
        return unpack_rows(T.tail_keep_mask(p, seed, offset, R, H), pl["seq_off"], pl["seq_kept"], L, True)

    masks["embeddings"] = remapped(first_offset)
    off = first_offset
    for i in range(cfg["N"] - 1):
        att = masks["layers"][i][0]
        masks["layers"][i] = (att, remapped(off + 2), remapped(off + 3))
        off += 3
    return masks


def calls_packed_masks(p, seed, first_offset, cfg, calls, rows):
    """packed_masks of every call of a step (rows: the capacity of each call): consecutive blocks of 1 + 3 N offsets."""
    if not p > 0:
        return [None] * len(calls)
    return [packed_masks(p, seed, first_offset + k * S.draws_per_call(cfg), cfg, c["lens"], c["ids"].shape[1], R)
            for k, (c, R) in enumerate(zip(calls, rows))]
