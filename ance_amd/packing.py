"""Packed token rows of a fixed capacity (csrc/pack_rows.hip behind ance_pack_tokens / ance_first_rows_*).

    packed = pack_tokens(input_ids, lens_from_mask(attention_mask), rows, token_type_ids, position_mode, padding_idx)
    h0 = first_rows(h, packed)                                   # [B, H]: row seq_off[s] of h [R, H], differentiable

A right-padded batch ``[B, L]`` becomes ``R = rows`` token rows that hold the sequences back to back.  ``rows`` is the CALLER's
capacity: an int fixes every shape, so a step that packs can be captured and replayed on batches with other lengths; how many of the
R rows are in use is known on the device only, and nothing synchronises.  A sequence that does not fit (``off_s + len_s > R``; such
sequences are a suffix of the batch) is DROPPED: it owns no rows, ``seq_kept`` is -1 for it, ``dropped`` grows by one, and
``first_rows`` hands out a row of NaN for it, so the loss of such a step is NaN and a ``GradScaler`` skips it on the device.  Rows
``T .. R - 1`` that no sequence covers (slack rows) hold a pad token (include/ance_amd.h states what exactly).

``rows="exact"`` reads the total back (``int(lens.sum())``, at least 1): ONE SYNCHRONISATION per call.  It is for eager use and for
tests; a captured step needs an int.

    packed = pack_tokens_by_id(input_ids, rows, padding_idx, vocab_size, max_position)          # the SEED-Encoder's rule

packs by ID instead of by length (ance_pack_tokens_by_id, three launches): every id equal to ``padding_idx`` is left out wherever it
sits, and the positions count the ids that stay.  A sequence that BEGINS with the pad id is dropped like one that does not fit (its
first row would not be its first token), but keeps its place in ``seq_off``, so its neighbours are untouched.
"""
import collections
import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .attention import HALF_DTYPES, _custom_bwd, _custom_fwd_as_is, _int32, _rows

__all__ = ["PackedTokens", "PackRule", "pack_tokens", "pack_tokens_by_id", "first_rows"]

MAX_SEQ_LEN, MAX_SEQS = 512, 65535
ROW_DTYPES = dict(HALF_DTYPES)
ROW_DTYPES[torch.float32] = _lib.ANCE_DTYPE_F32


class PackRule(collections.namedtuple("PackRule", "position_mode padding_idx vocab max_pos")):
    """The rule a packed batch's positions were formed under: position_mode ("absolute" / "roberta"; "seed": packed by id, which only
    ``pack_tokens_by_id`` makes), padding_idx (-1: none) and the two table sizes the clamps used (2^31 - 1: no clamp).  A tower takes
    only batches made under its own rule."""
    __slots__ = ()

    @classmethod
    def of(cls, position_mode, padding_idx, vocab_size, max_position):
        return cls(position_mode, -1 if padding_idx is None else int(padding_idx), 0x7fffffff if vocab_size is None else int(vocab_size),
                   0x7fffffff if max_position is None else int(max_position))


class PackedTokens(object):
    """What ``pack_tokens`` and the packed gather (``ance_amd.batches.PackedBatches``) return.  Device tensors: ``ids``, ``type_ids``
    (or None), ``positions`` -- int32 [R]; ``seq_off`` int32 [B + 1] (a dropped sequence's entry is the total T, so the differences
    are the kept lengths); ``seq_kept`` int32 [B] (the kept length, -1: dropped); ``dropped`` int64 0-dim: the counter ``pack_tokens``
    added to, or this batch's own count from the packed gather.  Host values: ``rows`` = R, ``max_seq_len`` = L, ``rule`` (a
    ``PackRule``: what the positions were formed under), ``chunks`` (sequences per item: 1, or C for a MaxP document batch)."""
    __slots__ = ("ids", "type_ids", "positions", "seq_off", "seq_kept", "rows", "max_seq_len", "dropped", "rule", "chunks")

    def __init__(self, ids, type_ids, positions, seq_off, seq_kept, rows, max_seq_len, dropped, rule=None, chunks=1):
        self.ids, self.type_ids, self.positions, self.seq_off, self.seq_kept = ids, type_ids, positions, seq_off, seq_kept
        self.rows, self.max_seq_len, self.dropped, self.rule, self.chunks = rows, max_seq_len, dropped, rule, chunks

    @property
    def n_seq(self):
        return self.seq_kept.numel()


def _ids_matrix(t, what, like=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dim() != 2 or t.numel() == 0 or t.dtype not in (torch.int32, torch.int64):
        raise _lib.AnceLibraryError("%s must be a CUDA(HIP) int32 or int64 tensor [B, L]" % what)
    if like is not None and (t.shape != like.shape or t.device != like.device):
        raise _lib.AnceLibraryError("%s must be shaped like input_ids, on its device" % what)
    return t.to(torch.int32).contiguous()


def pack_tokens(input_ids, lens, rows, token_type_ids=None, position_mode="absolute", padding_idx=None, vocab_size=None,
                max_position=None, dropped=None):
    """The plan and the packed keys of a right-padded batch, in two launches: input_ids [B, L] (B <= 65535, L <= 512), lens [B] device
    integers (``lens_from_mask``; clamped into 0 .. L), rows an int capacity >= 1 or "exact" (synchronises).  position_mode and
    padding_idx are ``bert_embeddings``'s; vocab_size / max_position are the tables' row counts, against which the positions are
    formed and clamped exactly as ``bert_embeddings`` does (None: no clamp).  ``dropped``: a 0-dim int64 device tensor to add the
    number of dropped sequences to (None: a fresh zero).  Returns a PackedTokens."""
    ids = _ids_matrix(input_ids, "input_ids")
    types = _ids_matrix(token_type_ids, "token_type_ids", ids) if token_type_ids is not None else None
    B, L = ids.shape
    dev = ids.device
    if B > MAX_SEQS or L > MAX_SEQ_LEN:
        raise _lib.AnceLibraryError("input_ids: at most %d sequences of at most %d tokens, got %r" % (MAX_SEQS, MAX_SEQ_LEN, (B, L)))
    if position_mode not in _lib.EMBED_POSITION_MODES:
        raise _lib.AnceLibraryError("position_mode must be \"absolute\" or \"roberta\", got %r" % (position_mode,))
    pad = -1 if padding_idx is None else int(padding_idx)
    if position_mode == "roberta" and padding_idx is None:
        raise _lib.AnceLibraryError("position_mode \"roberta\" needs a padding_idx")
    vocab = 0x7fffffff if vocab_size is None else int(vocab_size)
    max_pos = 0x7fffffff if max_position is None else int(max_position)
    if pad < -1 or pad >= vocab:
        raise _lib.AnceLibraryError("padding_idx must be in [0, %d), got %r" % (vocab, padding_idx))
    lens = _int32(lens, "lens", B, dev)
    if isinstance(rows, str):
        if rows != "exact":
            raise _lib.AnceLibraryError("rows must be an int capacity or \"exact\", got %r" % (rows,))
        rows = max(1, int(lens.clamp(0, L).sum()))   # the one synchronisation
    rows = int(rows)
    if not 1 <= rows <= 0x7fffffff:
        raise _lib.AnceLibraryError("rows must be in 1 .. 2^31 - 1, got %r" % (rows,))
    if dropped is None:
        dropped = torch.zeros((), dtype=torch.int64, device=dev)
    elif not isinstance(dropped, torch.Tensor) or dropped.dtype != torch.int64 or dropped.numel() != 1 or dropped.device != dev:
        raise _lib.AnceLibraryError("dropped must be a one-element int64 tensor on %s" % (dev,))
    out_ids = torch.empty(rows, dtype=torch.int32, device=dev)
    out_types = torch.empty(rows, dtype=torch.int32, device=dev) if types is not None else None
    out_pos = torch.empty(rows, dtype=torch.int32, device=dev)
    seq_off = torch.empty(B + 1, dtype=torch.int32, device=dev)
    seq_kept = torch.empty(B, dtype=torch.int32, device=dev)
    args = _lib.AncePackArgs(ids=ids.data_ptr(), type_ids=types.data_ptr() if types is not None else None, d_seq_len=lens.data_ptr(),
                             d_seq_off=seq_off.data_ptr(), d_seq_kept=seq_kept.data_ptr(), d_dropped=dropped.data_ptr(),
                             packed_ids=out_ids.data_ptr(), packed_type_ids=out_types.data_ptr() if types is not None else None,
                             packed_positions=out_pos.data_ptr(), n_seq=B, L=L, rows=rows,
                             position_mode=_lib.EMBED_POSITION_MODES[position_mode], padding_idx=pad, vocab=vocab, max_pos=max_pos)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ance_pack_tokens(ctypes.byref(args), _lib.current_stream_ptr()), "ance_pack_tokens")
    return PackedTokens(out_ids, out_types, out_pos, seq_off, seq_kept, rows, L, dropped,
                        PackRule.of(position_mode, padding_idx, vocab_size, max_position))


def pack_tokens_by_id(input_ids, rows, padding_idx, vocab_size=None, max_position=None, dropped=None):
    """``pack_tokens`` for a batch whose pad ids may sit anywhere in a row, in three launches: input_ids [B, L] (B <= 65535, L <= 512),
    rows an int capacity >= 1 or "exact" (synchronises once, on the count's result; at least 1), padding_idx the id to leave out.
    Positions are ``padding_idx + 1 + rank`` among the ids that stay, clamped into ``max_position`` rows (None: no clamp).  A
    sequence that begins with the pad id is dropped whatever the capacity (``seq_kept`` -1, counted in ``dropped``, NaN from
    ``first_rows``) and owns no rows.  Returns a PackedTokens without type ids under the rule ("seed", padding_idx, ...)."""
    ids = _ids_matrix(input_ids, "input_ids")
    B, L = ids.shape
    dev = ids.device
    if B > MAX_SEQS or L > MAX_SEQ_LEN:
        raise _lib.AnceLibraryError("input_ids: at most %d sequences of at most %d tokens, got %r" % (MAX_SEQS, MAX_SEQ_LEN, (B, L)))
    vocab = 0x7fffffff if vocab_size is None else int(vocab_size)
    max_pos = 0x7fffffff if max_position is None else int(max_position)
    if padding_idx is None or isinstance(padding_idx, bool) or not 0 <= int(padding_idx) < vocab:
        raise _lib.AnceLibraryError("padding_idx must be in [0, %d), got %r" % (vocab, padding_idx))
    pad = int(padding_idx)
    exact = isinstance(rows, str)
    if exact:
        if rows != "exact":
            raise _lib.AnceLibraryError("rows must be an int capacity or \"exact\", got %r" % (rows,))
        rows = 1   # the plan of this call is thrown away: only the count is read
    rows = int(rows)
    if not 1 <= rows <= 0x7fffffff:
        raise _lib.AnceLibraryError("rows must be in 1 .. 2^31 - 1, got %r" % (rows,))
    if dropped is None:
        dropped = torch.zeros((), dtype=torch.int64, device=dev)
    elif not isinstance(dropped, torch.Tensor) or dropped.dtype != torch.int64 or dropped.numel() != 1 or dropped.device != dev:
        raise _lib.AnceLibraryError("dropped must be a one-element int64 tensor on %s" % (dev,))
    lens = torch.empty(B, dtype=torch.int32, device=dev)
    seq_off = torch.empty(B + 1, dtype=torch.int32, device=dev)
    seq_kept = torch.empty(B, dtype=torch.int32, device=dev)

    def launch(rows, counter):
        out_ids = torch.empty(rows, dtype=torch.int32, device=dev)
        out_pos = torch.empty(rows, dtype=torch.int32, device=dev)
        args = _lib.AncePackByIdArgs(ids=ids.data_ptr(), d_seq_len=lens.data_ptr(), d_seq_off=seq_off.data_ptr(),
                                     d_seq_kept=seq_kept.data_ptr(), d_dropped=counter.data_ptr(), packed_ids=out_ids.data_ptr(),
                                     packed_positions=out_pos.data_ptr(), n_seq=B, L=L, rows=rows, padding_idx=pad, vocab=vocab,
                                     max_pos=max_pos)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().ance_pack_tokens_by_id(ctypes.byref(args), _lib.current_stream_ptr()), "ance_pack_tokens_by_id")
        return out_ids, out_pos

    if exact:
        launch(1, torch.zeros((), dtype=torch.int64, device=dev))   # the count alone matters; the caller's counter is not touched
        rows = max(1, int(lens.clamp(min=0).sum()))   # the one synchronisation
    out_ids, out_pos = launch(rows, dropped)
    return PackedTokens(out_ids, None, out_pos, seq_off, seq_kept, rows, L, dropped, PackRule.of("seed", pad, vocab_size, max_position))


def _first_rows_args(rows_matrix, ld_rows, first, packed):
    return _lib.AnceFirstRowsArgs(rows_matrix=rows_matrix.data_ptr(), first=first.data_ptr(), d_seq_off=packed.seq_off.data_ptr(),
                                  d_seq_kept=packed.seq_kept.data_ptr(), ld_rows=ld_rows, ld_first=first.shape[1],
                                  n_seq=first.shape[0], rows=rows_matrix.shape[0], H=first.shape[1],
                                  dtype=ROW_DTYPES[rows_matrix.dtype])


class _FirstRows(torch.autograd.Function):
    """x [R, H] fp32, fp16 or bf16 as it is -> [B, H] of the same dtype; the backward scatters into a zero-filled [R, H]."""

    @staticmethod
    @_custom_fwd_as_is
    def forward(ctx, x, packed):
        x, ld = _rows(x, 4 if x.dtype == torch.float32 else 8)
        out = torch.empty((packed.n_seq, x.shape[1]), dtype=x.dtype, device=x.device)
        args = _first_rows_args(x, ld, out, packed)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().ance_first_rows_gather(ctypes.byref(args), _lib.current_stream_ptr()), "ance_first_rows_gather")
        ctx.packed, ctx.shape, ctx.dtype = packed, x.shape, x.dtype
        return out

    @staticmethod
    @_custom_bwd
    @once_differentiable
    def backward(ctx, dout):
        dout = dout.to(ctx.dtype).contiguous()
        if dout.data_ptr() % 16:
            dout = dout.clone()
        dx = torch.zeros(ctx.shape, dtype=ctx.dtype, device=dout.device)   # one owner per first row; every other row stays zero
        args = _first_rows_args(dx, dx.shape[1], dout, ctx.packed)
        with torch.cuda.device(dout.device):
            _lib.check(_lib.lib().ance_first_rows_scatter(ctypes.byref(args), _lib.current_stream_ptr()), "ance_first_rows_scatter")
        return dx, None


def first_rows(x, packed):
    """[B, H]: row ``seq_off[s]`` of x [R, H] (fp32, fp16 or bf16; H 768 or 1024) for every kept sequence of length >= 1, a row of
    zeros for an empty one and a row of NaN for a dropped one.  The gradient of x is zero outside the first rows, an empty or a
    dropped sequence contributes nothing to it, and no two sequences share a row: no atomics, the same inputs give the same bits."""
    if not isinstance(packed, PackedTokens):
        raise _lib.AnceLibraryError("first_rows: packed must be a PackedTokens")
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() != 2 or x.dtype not in ROW_DTYPES or x.shape[1] not in (768, 1024):
        raise _lib.AnceLibraryError("first_rows: x must be a CUDA(HIP) tensor [R, 768 or 1024] of fp32, fp16 or bf16")
    if x.shape[0] != packed.rows or x.device != packed.seq_off.device:
        raise _lib.AnceLibraryError("first_rows: x must have the packed batch's %d rows, on its device; got %r" % (packed.rows, tuple(x.shape)))
    return _FirstRows.apply(x, packed)
