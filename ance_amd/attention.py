"""The trainers' self-attention core, differentiable (csrc/attention_train_kernels.h behind ance_attention_forward / _backward).

What transformers' eager ``BertSelfAttention.forward`` computes between its three Linear outputs and ``context_layer``, for
right-padded sequences and heads of width 64: scores * 0.125, softmax over the valid keys in fp32, dropout on the probabilities,
probabilities times values.  Nothing of size L^2 is stored: the forward keeps one log-sum-exp per (head, row), the backward
recomputes the probabilities and regenerates the dropout mask.  Pad query rows of the result and of the three gradients are zeros;
a sequence of length 0 is skipped.

    ctx = attention_padded(q, k, v, lens_from_mask(attention_mask), n_heads, dropout_p, self.training)     # [B, L, H] each
    ctx = attention_packed(q, k, v, seq_off, max_seq_len, n_heads, dropout_p, self.training)               # [T, H] each

Dropout: Philox4x32-10 under (seed, offset), stated in include/ance_amd.h.  ``seed`` is ``manual_seed(n)``'s (default:
``torch.initial_seed()``, read on the host when first needed); ``offset`` is a per-device call counter that every dropout forward
advances by one.  The backward gets the forward's pair through the autograd context.  By default both are HOST values baked into
the launch: a captured graph replays the pair it was captured with -- the same mask at every replay.  The masks are not torch's.

``dropout_state.to_device()`` opts a device into the device-resident stream: its counter moves into a device tensor {seed, base}
that every dropout kernel reads at its entry, a call draws under ``base + r`` (r: calls since the last ``advance``), and
``dropout_state.advance()`` -- once per step, after the backward, inside a captured region -- adds the step's calls to the base.
Eager code draws the same masks as in host mode; a replayed graph draws the masks of the step it stands for.
"""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib

try:  # torch >= 2.4
    from torch.amp import custom_bwd as _amp_bwd, custom_fwd as _amp_fwd
    _custom_fwd = _amp_fwd(device_type="cuda", cast_inputs=torch.float32)
    _custom_fwd_as_is = _amp_fwd(device_type="cuda")   # precision="half": the inputs go in as they are
    _custom_bwd = _amp_bwd(device_type="cuda")
except ImportError:  # pragma: no cover
    from torch.cuda.amp import custom_bwd as _custom_bwd, custom_fwd as _amp_fwd
    _custom_fwd = _amp_fwd(cast_inputs=torch.float32)
    _custom_fwd_as_is = _amp_fwd

__all__ = ["attention_padded", "attention_packed", "attention_first_row", "attention_first_row_packed", "lens_from_mask",
           "manual_seed", "dropout_state"]


class _Draw(object):
    """What one dropout forward draws under and its backward keeps: the host pair ``(seed, offset)``, or -- in device mode --
    ``stream`` (the device tensor {seed, base}), ``offset`` = the call's index r within the step and the epoch of the stream."""
    __slots__ = ("state", "dev", "seed", "offset", "stream", "epoch")

    def __init__(self, state, dev, seed, offset, stream, epoch):
        self.state, self.dev, self.seed, self.offset, self.stream, self.epoch = state, dev, seed, offset, stream, epoch

    def launch(self, name, *structs):
        """The entry point ``name`` on the current stream, or its ``_dstream`` sibling in device mode.  A backward whose base has
        moved since its forward (``advance``, ``manual_seed``, ``to_host``) would regenerate another mask: it is refused."""
        L = _lib.lib()
        if self.stream is None:
            _lib.check(getattr(L, name)(*structs, _lib.current_stream_ptr()), name)
            return
        if self.state.epochs.get(self.dev) != self.epoch:
            raise _lib.AnceLibraryError("%s: the device dropout stream has moved since this call's forward (dropout_state.advance, "
                                        "manual_seed or to_host ran in between): the backward would regenerate another mask; call "
                                        "advance() once per step, after the backward" % name)
        name += "_dstream"
        _lib.check(getattr(L, name)(*structs, ctypes.c_void_p(self.stream.data_ptr()), _lib.current_stream_ptr()), name)


def _as_int64(n):
    return n - (1 << 64) if n >= 1 << 63 else n


class _DropoutState:
    """The seed and the per-device call counters of the dropout stream.  Host values by default.  After ``to_device`` a device's
    counter lives in a 2-element int64 device tensor {seed, base}, which every dropout kernel reads at its entry: the effective
    offset of a call is ``base + r``, r counting the calls since the last ``advance``, so an eager program draws the same masks in
    both modes whether or not it calls ``advance``, and a captured step that ends with ``advance`` draws the masks of the step it
    stands for at every replay."""

    def __init__(self):
        self.seed = None
        self.offsets = {}   # host mode: calls so far; device mode: r, the calls since the last advance
        self.streams = {}   # device index -> the device tensor {seed, base} while that device is in device mode
        self.epochs = {}    # device index -> how often its base has moved under the autograd contexts (advance, manual_seed, to_host)
        self._tensors = {}  # every tensor ever handed out, kept so that a captured graph's pointer stays valid and is reused

    def _seed(self):
        if self.seed is None:
            self.seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        return self.seed

    @staticmethod
    def _index(device):
        if device is None:
            return torch.cuda.current_device()
        if isinstance(device, int):
            return device
        device = torch.device(device)
        return device.index if device.index is not None else torch.cuda.current_device()

    def _write(self, dev, seed, base):
        """{seed, base} into the device's tensor: a host-to-device copy, not capturable."""
        t = self._tensors.get(dev)
        if t is None:
            t = self._tensors[dev] = torch.zeros(2, dtype=torch.int64, device=torch.device("cuda", dev))
            if t.data_ptr() % 16:
                raise _lib.AnceLibraryError("the device dropout stream must be 16-byte aligned")
        t.copy_(torch.tensor([_as_int64(seed), _as_int64(base & 0xFFFFFFFFFFFFFFFF)], dtype=torch.int64))
        return t

    def manual_seed(self, n):
        """Host mode: as before.  Device mode: rewrites every device tensor to {n, 0} -- a copy from the host, NOT capturable."""
        self.seed = int(n) & 0xFFFFFFFFFFFFFFFF
        self.offsets = {}
        for dev in self.streams:
            self._write(dev, self.seed, 0)
            self.epochs[dev] = self.epochs.get(dev, 0) + 1

    def to_device(self, device=None):
        """Moves ``device``'s counter into its device tensor {seed, calls so far} and returns the tensor.  From then on
        ``next_pair`` hands out ``(d_stream, r)``.  One small copy from the host: call it before capturing."""
        dev = self._index(device)
        if dev not in self.streams:
            self.streams[dev] = self._write(dev, self._seed(), self.offsets.get(dev, 0))
            self.offsets[dev] = 0
            self.epochs[dev] = self.epochs.get(dev, 0) + 1
        return self.streams[dev]

    def to_host(self, device=None):
        """``(seed, calls so far)`` of ``device``, read back for checkpointing, and the device is in host mode again (``to_device``
        returns to the same tensor, so a captured graph stays valid).  ONE SYNCHRONISING READ: off the step path."""
        dev = self._index(device)
        if dev in self.streams:
            seed, base = self.streams.pop(dev).tolist()
            self.seed = seed & 0xFFFFFFFFFFFFFFFF
            self.offsets[dev] = (base & 0xFFFFFFFFFFFFFFFF) + self.offsets.get(dev, 0)
            self.epochs[dev] = self.epochs.get(dev, 0) + 1
        return self._seed(), self.offsets.get(dev, 0)

    def advance(self, device=None):
        """Device mode: enqueues ``base += r`` (one one-thread kernel, capturable) and resets r; nothing when r is 0 or in host mode.
        Once per step, AFTER the backward: a backward that runs behind it is refused (its masks would be another step's)."""
        dev = self._index(device)
        r = self.offsets.get(dev, 0)
        if dev not in self.streams or r == 0:
            return
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().ance_dropout_stream_advance(ctypes.c_void_p(self.streams[dev].data_ptr()), r, _lib.current_stream_ptr()),
                       "ance_dropout_stream_advance")
        self.offsets[dev] = 0
        self.epochs[dev] += 1

    def next_pair(self, device):
        """Host mode: ``(seed, offset)``; device mode: ``(d_stream, r)``.  Either way the device's call counter grows by one."""
        seed = self._seed()
        dev = self._index(device)
        off = self.offsets.get(dev, 0)
        self.offsets[dev] = off + 1
        stream = self.streams.get(dev)
        return (seed, off) if stream is None else (stream, off)

    def draw(self, device):
        """``next_pair`` as the autograd functions keep it (``_Draw``)."""
        a, off = self.next_pair(device)
        dev = self._index(device)
        if isinstance(a, torch.Tensor):
            return _Draw(self, dev, 0, off, a, self.epochs[dev])
        return _Draw(self, dev, a, off, None, 0)


dropout_state = _DropoutState()
_NO_DRAW = _Draw(dropout_state, -1, 0, 0, None, 0)   # a call without dropout


def manual_seed(n):
    """Seeds the dropout stream and resets every device's call counter: the same calls after it give the same bits.  In device mode
    (``dropout_state.to_device``) it rewrites the device tensors with a copy from the host, so it cannot be captured."""
    dropout_state.manual_seed(n)


def lens_from_mask(attention_mask):
    """[B] int32 lengths of a [B, L] attention mask, computed on the device with no synchronisation.  The mask must be a right-padded
    prefix (ones, then zeros), as every loader of the reference produces; a mask with holes is outside the contract -- it is read as
    the prefix with the same number of ones."""
    if attention_mask.dim() != 2:
        raise _lib.AnceLibraryError("attention_mask must be [B, L]")
    return (attention_mask != 0).sum(dim=1, dtype=torch.int32)


def _rows(t, piece=4):
    """A [.., H] CUDA tensor as a row matrix: (tensor to keep alive, row stride).  The kernels read 16-byte pieces, so a row stride
    must be a multiple of ``piece`` elements: 4 for fp32, 8 for a 16-bit dtype.  A view whose rows are evenly spaced passes as it is;
    anything else is copied."""
    if t.dim() == 3:
        if t.stride(2) != 1 or t.stride(0) != t.size(1) * t.stride(1) or t.stride(1) % piece or t.stride(1) < t.size(2) \
                or t.data_ptr() % 16:
            t = t.contiguous()
        return t, t.stride(1)
    if t.stride(1) != 1 or t.stride(0) % piece or t.stride(0) < t.size(1) or t.data_ptr() % 16:
        t = t.contiguous()
    return t, t.stride(0)


HALF_DTYPES = {torch.float16: _lib.ANCE_DTYPE_F16, torch.bfloat16: _lib.ANCE_DTYPE_BF16}


def _check_precision(precision):
    if precision not in ("fp32", "half"):
        raise _lib.AnceLibraryError("precision must be \"fp32\" or \"half\", got %r" % (precision,))
    return precision == "half"


def _check_inputs(q, k, v, n_heads, dropout_p, dims, half=False):
    for t, what in ((q, "q"), (k, "k"), (v, "v")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.AnceLibraryError("%s must be a CUDA(HIP) tensor" % what)
        if half:  # precision="half": fp16 or bf16 as they are; fp32 only under autocast, which casts it (_half_inputs)
            if t.dtype not in HALF_DTYPES and not (torch.is_autocast_enabled() and t.dtype == torch.float32):
                raise _lib.AnceLibraryError("%s must have dtype torch.float16 or bfloat16 with precision=\"half\", got %s"
                                            % (what, t.dtype))
        elif t.dtype != torch.float32 and not (torch.is_autocast_enabled() and t.is_floating_point()):  # autocast: cast below
            raise _lib.AnceLibraryError("%s must have dtype torch.float32, got %s" % (what, t.dtype))
        if t.dim() != dims or t.shape != q.shape or t.device != q.device:
            raise _lib.AnceLibraryError("q, k, v must be %d-dimensional, of one shape, on one device" % dims)
    if n_heads not in (12, 16):
        raise _lib.AnceLibraryError("n_heads must be 12 or 16, got %r" % (n_heads,))
    if q.shape[-1] != 64 * n_heads:
        raise _lib.AnceLibraryError("the last dimension must be 64 * n_heads = %d, got %d" % (64 * n_heads, q.shape[-1]))
    if not 0.0 <= float(dropout_p) < 1.0:
        raise _lib.AnceLibraryError("dropout_p must be in [0, 1), got %r" % (dropout_p,))
    if q.numel() == 0:
        raise _lib.AnceLibraryError("empty input")


def _int32(t, what, n, device):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != device or t.dim() != 1 or t.numel() != n \
            or t.dtype not in (torch.int32, torch.int64):
        raise _lib.AnceLibraryError("%s must be a device integer tensor [%d] on %s" % (what, n, device))
    return t.to(torch.int32).contiguous()


def _grads_like(q, k, v, zero):
    """Gradients in the inputs' own strides (zeroed for the packed form; in the padded form the kernels write every row).  Views of
    one fused buffer ([.., 3H] rows) get views of one fused gradient."""
    ts = (q, k, v)
    make = torch.zeros if zero else torch.empty
    if all(t.is_contiguous() for t in ts):
        return tuple(make(t.shape, dtype=t.dtype, device=t.device) for t in ts)
    H, ld = q.shape[-1], q.stride(-2)
    same = all(t.stride() == q.stride() and t.untyped_storage().data_ptr() == q.untyped_storage().data_ptr() for t in ts)
    offs = [t.storage_offset() for t in ts]
    if same and ld >= 3 * H and max(offs) - min(offs) + H <= ld and offs[0] // ld == offs[1] // ld == offs[2] // ld:
        base = min(offs)
        fused = torch.zeros(q.shape[:-1] + (ld,), dtype=q.dtype, device=q.device) if zero or ld > 3 * H else \
            torch.empty(q.shape[:-1] + (ld,), dtype=q.dtype, device=q.device)
        return tuple(fused[..., o - base:o - base + H] for o in offs)
    out = tuple(torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=t.device) for t in ts)
    return tuple(t.zero_() for t in out) if zero else out


def _core_forward(ctx, q, k, v, first, lens, max_seq_len, n_heads, dropout_p, training, half):
    """The forward of both full-core functions (csrc/attention_train_kernels.h): q, k, v [B, L, H] or [T, H] of one dtype -- fp32, or
    with ``half`` fp16 / bf16."""
    L = _lib.lib()
    piece, entry = (8, "ance_attention16") if half else (4, "ance_attention")
    (q, ld_q), (k, ld_k), (v, ld_v) = _rows(q, piece), _rows(k, piece), _rows(v, piece)
    n_rows = q.numel() // q.shape[-1]
    # padded form: the kernels write the pad rows' zeros themselves; packed form: rows that no sequence covers stay zero
    seq_rows = max_seq_len if q.dim() == 3 else 0
    out = (torch.empty if seq_rows else torch.zeros)(q.shape, dtype=q.dtype, device=q.device)
    ws_bytes = getattr(L, entry + "_workspace_bytes")(n_rows, n_heads)
    if ws_bytes == 0:
        raise _lib.AnceLibraryError("attention: unsupported shape (rows %d, heads %d)" % (n_rows, n_heads))
    ws = torch.zeros(ws_bytes // 4, dtype=torch.float32, device=q.device)
    drop = bool(training) and dropout_p > 0.0
    draw = dropout_state.draw(q.device) if drop else _NO_DRAW
    common = dict(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), ctx=out.data_ptr(), ld_q=ld_q, ld_k=ld_k, ld_v=ld_v,
                  ld_ctx=out.shape[-1], d_seq_first=first.data_ptr(), d_seq_len=lens.data_ptr(), n_seq=first.numel(),
                  max_seq_len=max_seq_len, n_rows=n_rows, n_heads=n_heads, seq_rows=seq_rows, dropout_p=float(dropout_p),
                  training=1 if drop else 0, seed=draw.seed, offset=draw.offset, d_workspace=ws.data_ptr(), workspace_bytes=ws_bytes)
    args = _lib.AnceAttn16Args(dtype=HALF_DTYPES[q.dtype], **common) if half else _lib.AnceAttnTrainArgs(**common)
    with torch.cuda.device(q.device):
        draw.launch(entry + "_forward", ctypes.byref(args))
    ctx.save_for_backward(q, k, v, out, first, lens, ws)
    ctx.args, ctx.draw = args, draw
    lse = ws[:n_heads * n_rows].view(n_heads, n_rows)
    ctx.mark_non_differentiable(lse)
    return out, lse


def _core_backward(ctx, dctx, half):
    q, k, v, out, first, lens, ws = ctx.saved_tensors
    a = ctx.args
    dctx, ld_d = _rows(dctx.to(q.dtype), 8 if half else 4)
    dq, dk, dv = _grads_like(q, k, v, zero=a.seq_rows == 0)
    g = (_lib.AnceAttn16GradArgs if half else _lib.AnceAttnGradArgs)(
        dctx=dctx.data_ptr(), dq=dq.data_ptr(), dk=dk.data_ptr(), dv=dv.data_ptr(), ld_dctx=ld_d, ld_dq=dq.stride(-2),
        ld_dk=dk.stride(-2), ld_dv=dv.stride(-2))
    with torch.cuda.device(q.device):
        ctx.draw.launch("ance_attention16_backward" if half else "ance_attention_backward", ctypes.byref(a), ctypes.byref(g))
    return dq, dk, dv, None, None, None, None, None, None


class _Attention(torch.autograd.Function):
    """q, k, v: [B, L, H] or [T, H] fp32 (autocast casts them); first, lens: int32 [n_seq] on the device."""

    @staticmethod
    @_custom_fwd
    def forward(ctx, q, k, v, first, lens, max_seq_len, n_heads, dropout_p, training):
        return _core_forward(ctx, q, k, v, first, lens, max_seq_len, n_heads, dropout_p, training, False)

    @staticmethod
    @_custom_bwd
    @once_differentiable
    def backward(ctx, dctx, _dlse):
        return _core_backward(ctx, dctx, False)


class _AttentionHalf(torch.autograd.Function):
    """_Attention with fp16 / bf16 rows: nothing is cast, ctx and the gradients have the inputs' dtype, the log-sum-exp stays fp32."""

    @staticmethod
    @_custom_fwd_as_is
    def forward(ctx, q, k, v, first, lens, max_seq_len, n_heads, dropout_p, training):
        return _core_forward(ctx, q, k, v, first, lens, max_seq_len, n_heads, dropout_p, training, True)

    @staticmethod
    @_custom_bwd
    @once_differentiable
    def backward(ctx, dctx, _dlse):
        return _core_backward(ctx, dctx, True)


def _half_inputs(q, k, v):
    """precision="half": under autocast fp32 inputs are cast to the autocast dtype (a differentiable cast, as autocast's own); then
    all three must be of one 16-bit dtype."""
    if torch.is_autocast_enabled():
        to = torch.get_autocast_dtype("cuda") if hasattr(torch, "get_autocast_dtype") else torch.get_autocast_gpu_dtype()
        q, k, v = (t.to(to) if t.dtype == torch.float32 else t for t in (q, k, v))
    if q.dtype not in HALF_DTYPES or k.dtype != q.dtype or v.dtype != q.dtype:
        raise _lib.AnceLibraryError("q, k, v must all be torch.float16 or all bfloat16 with precision=\"half\", got %s, %s, %s"
                                    % (q.dtype, k.dtype, v.dtype))
    return q, k, v


def _padded(q, k, v, lens, n_heads, dropout_p, training, precision="fp32"):
    half = _check_precision(precision)
    _check_inputs(q, k, v, n_heads, dropout_p, 3, half)
    B, Lq = q.shape[0], q.shape[1]
    if not 1 <= Lq <= 512:
        raise _lib.AnceLibraryError("sequence length must be in 1 .. 512, got %d" % Lq)
    lens = _int32(lens, "lens", B, q.device)
    first = torch.arange(0, B * Lq, Lq, dtype=torch.int32, device=q.device)
    if half:
        return _AttentionHalf.apply(*_half_inputs(q, k, v), first, lens, Lq, n_heads, float(dropout_p), bool(training))
    return _Attention.apply(q, k, v, first, lens, Lq, n_heads, float(dropout_p), bool(training))


def _packed(q, k, v, seq_off, max_seq_len, n_heads, dropout_p, training, precision="fp32"):
    half = _check_precision(precision)
    _check_inputs(q, k, v, n_heads, dropout_p, 2, half)
    if not 1 <= int(max_seq_len) <= 512:
        raise _lib.AnceLibraryError("max_seq_len must be in 1 .. 512, got %r" % (max_seq_len,))
    if not isinstance(seq_off, torch.Tensor) or seq_off.dim() != 1 or seq_off.numel() < 2:
        raise _lib.AnceLibraryError("seq_off must be a device integer tensor [n_seq + 1]")
    off = _int32(seq_off, "seq_off", seq_off.numel(), q.device)
    first, lens = off[:-1].contiguous(), (off[1:] - off[:-1]).contiguous()
    if half:
        return _AttentionHalf.apply(*_half_inputs(q, k, v), first, lens, int(max_seq_len), n_heads, float(dropout_p), bool(training))
    return _Attention.apply(q, k, v, first, lens, int(max_seq_len), n_heads, float(dropout_p), bool(training))


def _first_row_forward(ctx, q0, k, v, first, lens, n_heads, dropout_p, training, max_seq_len, piece, dtype_code):
    """The forward of both first-row functions (csrc/attention_row0.hip): q0 [B, H], k, v of one dtype -- [B, L, H] (the padded form,
    max_seq_len = L) or [R, H] (the packed form: seq_rows = 0, nothing outside the valid rows is written)."""
    L = _lib.lib()
    (q0, ld_q), (k, ld_k), (v, ld_v) = _rows(q0, piece), _rows(k, piece), _rows(v, piece)
    B, H = q0.shape
    Lk, n_rows, seq_rows = max_seq_len, k.numel() // H, max_seq_len if k.dim() == 3 else 0
    out = torch.empty((B, H), dtype=q0.dtype, device=q0.device)
    ws_bytes = L.ance_attention_row0_workspace_bytes(B, n_heads)
    if ws_bytes == 0:
        raise _lib.AnceLibraryError("attention_first_row: unsupported shape (sequences %d, heads %d)" % (B, n_heads))
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=q0.device)   # (max, sum) per (sequence, head)
    drop = bool(training) and dropout_p > 0.0
    draw = dropout_state.draw(q0.device) if drop else _NO_DRAW
    args = _lib.AnceAttn16Args(q=q0.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), ctx=out.data_ptr(), ld_q=ld_q, ld_k=ld_k, ld_v=ld_v,
                               ld_ctx=H, d_seq_first=first.data_ptr(), d_seq_len=lens.data_ptr(), n_seq=B, max_seq_len=Lk,
                               n_rows=n_rows, n_heads=n_heads, seq_rows=seq_rows, dtype=dtype_code, dropout_p=float(dropout_p),
                               training=1 if drop else 0, seed=draw.seed, offset=draw.offset, d_workspace=ws.data_ptr(),
                               workspace_bytes=ws_bytes)
    with torch.cuda.device(q0.device):
        draw.launch("ance_attention_row0_forward", ctypes.byref(args))
    ctx.save_for_backward(q0, k, v, first, lens, ws)
    ctx.args, ctx.draw = args, draw
    return out


def _first_row_backward(ctx, dctx0, piece):
    q0, k, v, first, lens, ws = ctx.saved_tensors
    dctx0, ld_d = _rows(dctx0.to(q0.dtype), piece)
    dq0 = torch.empty(q0.shape, dtype=q0.dtype, device=q0.device)
    # padded form: the kernel writes every row, pads as zeros; packed form: rows that no sequence covers stay zero
    make = torch.empty if ctx.args.seq_rows else torch.zeros
    dk, dv = (make(k.shape, dtype=k.dtype, device=k.device) for _ in range(2))
    g = _lib.AnceAttn16GradArgs(dctx=dctx0.data_ptr(), dq=dq0.data_ptr(), dk=dk.data_ptr(), dv=dv.data_ptr(), ld_dctx=ld_d,
                                ld_dq=dq0.shape[-1], ld_dk=dk.shape[-1], ld_dv=dv.shape[-1])
    with torch.cuda.device(q0.device):
        ctx.draw.launch("ance_attention_row0_backward", ctypes.byref(ctx.args), ctypes.byref(g))
    return dq0, dk, dv, None, None, None, None, None, None


class _AttentionFirstRow(torch.autograd.Function):
    """q0 [B, H], k, v [B, L, H] fp32; first, lens: int32 [B] on the device."""

    @staticmethod
    @_custom_fwd
    def forward(ctx, q0, k, v, first, lens, n_heads, dropout_p, training, max_seq_len):
        return _first_row_forward(ctx, q0, k, v, first, lens, n_heads, dropout_p, training, max_seq_len, 4, _lib.ANCE_DTYPE_F32)

    @staticmethod
    @_custom_bwd
    @once_differentiable
    def backward(ctx, dctx0):
        return _first_row_backward(ctx, dctx0, 4)


class _AttentionFirstRowHalf(torch.autograd.Function):
    """_AttentionFirstRow with fp16 / bf16 rows: nothing is cast, ctx0 and the gradients have the inputs' dtype."""

    @staticmethod
    @_custom_fwd_as_is
    def forward(ctx, q0, k, v, first, lens, n_heads, dropout_p, training, max_seq_len):
        return _first_row_forward(ctx, q0, k, v, first, lens, n_heads, dropout_p, training, max_seq_len, 8, HALF_DTYPES[q0.dtype])

    @staticmethod
    @_custom_bwd
    @once_differentiable
    def backward(ctx, dctx0):
        return _first_row_backward(ctx, dctx0, 8)


def attention_first_row(q0, k, v, lens, n_heads, dropout_p=0.0, training=True, precision="fp32"):
    """ctx0 [B, H]: row 0 of ``attention_padded(q, k, v, ...)`` from the first rows' queries alone -- q0 [B, H] (= q[:, 0]), k, v
    [B, L, H], lens [B] device integers (lens_from_mask), L <= 512.  What a tower's last layer needs when only h[:, 0] is read: one
    memory-bound pass over k and v per (sequence, head) instead of an L x L core (csrc/attention_row0.hip).  Views with a contiguous
    last dimension and evenly spaced rows pass as they are (thirds of a fused [B, L, 3H]; hidden[:, 0]).  Gradients for q0, k and v;
    rows >= lens[b] of dk and dv are zeros; a sequence of length 0 gives a zero ctx0 row and zero gradients.  Under the same (seed,
    offset) the dropout mask is the full core's query row 0, bit for bit; the call takes one draw of the dropout stream.
    precision="half": q0, k, v all fp16 or all bf16 (under autocast fp32 ones are cast to the autocast dtype; outside it they are
    refused); the arithmetic is fp32 and every output is rounded once, at its store.  The default casts to fp32 under autocast and
    refuses 16-bit inputs outside it."""
    half = _check_precision(precision)
    _check_inputs(k, k, v, n_heads, dropout_p, 3, half)
    _check_inputs(q0, q0, q0, n_heads, dropout_p, 2, half)
    B, Lk = k.shape[0], k.shape[1]
    if q0.shape[0] != B or q0.device != k.device:
        raise _lib.AnceLibraryError("q0 must be [B, H] with k's batch size, on k's device; got %r and %r" % (tuple(q0.shape), tuple(k.shape)))
    if not 1 <= Lk <= 512:
        raise _lib.AnceLibraryError("sequence length must be in 1 .. 512, got %d" % Lk)
    lens = _int32(lens, "lens", B, k.device)
    first = torch.arange(0, B * Lk, Lk, dtype=torch.int32, device=k.device)
    if half:
        return _AttentionFirstRowHalf.apply(*_half_inputs(q0, k, v), first, lens, n_heads, float(dropout_p), bool(training), Lk)
    return _AttentionFirstRow.apply(q0, k, v, first, lens, n_heads, float(dropout_p), bool(training), Lk)


def attention_first_row_packed(q0, k, v, seq_off, max_seq_len, n_heads, dropout_p=0.0, training=True, precision="fp32"):
    """``attention_first_row`` over packed rows: q0 [B, H] (the query of every sequence's first row), k, v [R, H], sequence s being
    rows seq_off[s] .. seq_off[s + 1] - 1 (seq_off: device integers [B + 1]), each at most max_seq_len <= 512 rows.  ctx0 [B, H];
    gradients for q0, k and v, of which dk and dv are zero at every row that no sequence covers.  A sequence of length 0 (an empty
    or a dropped one of ``pack_tokens``) gives a zero ctx0 row and zero gradients.  The dropout mask of sequence s is the padded
    call's, bit for bit, under the same (seed, offset).  precision: as attention_first_row."""
    half = _check_precision(precision)
    _check_inputs(k, k, v, n_heads, dropout_p, 2, half)
    _check_inputs(q0, q0, q0, n_heads, dropout_p, 2, half)
    if not 1 <= int(max_seq_len) <= 512:
        raise _lib.AnceLibraryError("max_seq_len must be in 1 .. 512, got %r" % (max_seq_len,))
    B = q0.shape[0]
    if q0.device != k.device or not isinstance(seq_off, torch.Tensor) or seq_off.dim() != 1 or seq_off.numel() != B + 1:
        raise _lib.AnceLibraryError("q0 must be [B, H] on k's device and seq_off a device integer tensor [B + 1]")
    off = _int32(seq_off, "seq_off", B + 1, k.device)
    first, lens = off[:-1].contiguous(), (off[1:] - off[:-1]).contiguous()
    if half:
        return _AttentionFirstRowHalf.apply(*_half_inputs(q0, k, v), first, lens, n_heads, float(dropout_p), bool(training),
                                            int(max_seq_len))
    return _AttentionFirstRow.apply(q0, k, v, first, lens, n_heads, float(dropout_p), bool(training), int(max_seq_len))


# _padded / _packed return (ctx, lse): lse is the saved fp32 log-sum-exp [n_heads, rows] (zeros at pad rows), non-differentiable.  It
# is not part of the interface; the tests read it.
def attention_padded(q, k, v, lens, n_heads, dropout_p=0.0, training=True, precision="fp32"):
    """ctx [B, L, H] of right-padded sequences: q, k, v [B, L, H] fp32 (views with a contiguous last dimension pass as they are, so
    three Linear outputs and the three thirds of a fused [B, L, 3H] both work), lens [B] device integers (lens_from_mask).  Rows
    >= lens[b] of ctx and of the gradients are zeros; L <= 512.
    precision="half": q, k, v all fp16 or all bf16 (under autocast fp32 ones are cast to the autocast dtype; outside it they are
    refused); the products run on the 16-bit matrix cores with fp32 softmax and accumulation, and ctx and the gradients have the
    inputs' dtype.  The default casts to fp32 under autocast and refuses 16-bit inputs outside it."""
    return _padded(q, k, v, lens, n_heads, dropout_p, training, precision)[0]


def attention_packed(q, k, v, seq_off, max_seq_len, n_heads, dropout_p=0.0, training=True, precision="fp32"):
    """ctx [T, H] of packed sequences: sequence s is rows seq_off[s] .. seq_off[s + 1] - 1 (seq_off: device integers [n_seq + 1]),
    each at most max_seq_len <= 512 rows (a longer one is cut there).  precision: as attention_padded."""
    return _packed(q, k, v, seq_off, max_seq_len, n_heads, dropout_p, training, precision)[0]
