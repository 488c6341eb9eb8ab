"""The row-wise seams of a BertLayer, differentiable (csrc/layer_tail.hip behind ance_layer_tail_* / ance_bias_gelu_*), and a
drop-in BertLayer built from them and the attention core.

    y = dropout_add_layer_norm(dense_out, dense.bias, input_tensor, LayerNorm.weight, LayerNorm.bias, eps, p, self.training)
    y = bias_gelu(dense_out, dense.bias)

``dropout_add_layer_norm`` is what transformers' eager ``BertSelfOutput.forward`` / ``BertOutput.forward`` compute after the dense
matmul -- ``LayerNorm(dropout(x + bias) + input_tensor)`` -- in one launch; it keeps two floats per row (mean, 1 / sqrt(var + eps))
and no mask: the backward recomputes the normalised row from its inputs and regenerates the mask.  ``bias_gelu`` is
``BertIntermediate.forward`` after its matmul, the erf form; it keeps nothing but its input.  The parameter gradients (weight, beta,
bias) are column sums without atomics: the same inputs give the same bits.

Dropout draws its (seed, offset) from ``ance_amd.attention.dropout_state`` -- the one stream that ``attention.manual_seed`` seeds and
that every dropout forward, the attention's included, advances by one, so no two calls share a pair.  A call with ``training`` false
or ``dropout_p == 0`` draws nothing.  By default both are HOST values baked into the launch: a captured graph replays the pair it was
captured with -- the same mask at every replay; ``dropout_state.to_device()`` moves the stream to the device, where a replayed
step draws the masks of the step it stands for (ance_amd/attention.py).  The masks are not torch's.

``precision="half"`` (both functions; ``BertLayer(..., precision="half")``) is the form for ``torch.autocast`` (csrc/layer_tail_half.hip
behind ance_layer_tail16_* / ance_bias_gelu16_*): the dense outputs go in as fp16 / bf16, the residual stream, ``y`` and every
parameter gradient stay fp32, and the tail can return a 16-bit copy of ``y`` for the Linears that read it.

Both precisions of a seam share one forward and one backward body (``_tail_forward`` ... ``_gelu_backward``, taking ``half``), and
the four forms of ``BertLayer`` -- all rows or first rows, padded or packed -- share one forward text (``BertLayer._layer``).
"""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .attention import (_NO_DRAW, HALF_DTYPES, _check_precision, _custom_bwd, _custom_fwd, _custom_fwd_as_is, _rows,
                        attention_first_row, attention_first_row_packed, attention_packed, attention_padded, dropout_state)
from .packing import PackedTokens, first_rows

__all__ = ["dropout_add_layer_norm", "bias_gelu", "BertLayer"]

TAIL_WIDTHS, GELU_WIDTHS = (768, 1024), (3072, 4096)


def _check_rows(t, what, widths):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.AnceLibraryError("%s must be a CUDA(HIP) tensor" % what)
    if t.dtype != torch.float32 and not (torch.is_autocast_enabled() and t.is_floating_point()):  # autocast: cast below
        raise _lib.AnceLibraryError("%s must have dtype torch.float32, got %s" % (what, t.dtype))
    if t.dim() < 2 or t.shape[-1] not in widths:
        raise _lib.AnceLibraryError("%s must be [.., W] with W in %r, got %r" % (what, widths, tuple(t.shape)))
    if t.numel() == 0:
        raise _lib.AnceLibraryError("empty input")


def _check_vector(t, what, width, like, optional=False):
    if t is None and optional:
        return
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != like.device or t.dim() != 1 or t.numel() != width:
        raise _lib.AnceLibraryError("%s must be a CUDA(HIP) tensor [%d] on %s" % (what, width, like.device))
    if t.dtype != torch.float32 and not (torch.is_autocast_enabled() and t.is_floating_point()):
        raise _lib.AnceLibraryError("%s must have dtype torch.float32, got %s" % (what, t.dtype))


def _matrix(t, piece=4):
    """[.., W] as (tensor to keep alive, row stride): 2- and 3-dimensional views with evenly spaced rows pass as they are.  piece:
    the elements of a 16-byte piece of a row, which the row stride must be a multiple of (4 for fp32, 8 for a 16-bit tensor)."""
    if t.dim() > 3:
        t = t.reshape(-1, t.shape[-1])
    return _rows(t, piece)


def _vector(t):
    """A [W] parameter as the kernels read it: contiguous and 16-byte aligned (a slice of a flat parameter buffer is copied)."""
    if t is None:
        return None
    t = t.detach()
    return t if t.is_contiguous() and t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _stats_floats(n_rows):
    """include/ance_amd.h: the saved state of the layer tail, mean [n_rows] and rstd [n_rows], each rounded up to 256 bytes."""
    return 2 * ((4 * n_rows + 255) // 256 * 256) // 4


# per precision (indexed by half): the elements of a 16-byte piece of x, the names of the workspace query, the forward and the backward
# entry, the argument and the gradient struct -- written out once here, so that a call looks nothing up but the library's attribute
_TAIL = ((4, "ance_layer_tail_workspace_bytes", "ance_layer_tail_forward", "ance_layer_tail_backward",
          _lib.AnceLayerTailArgs, _lib.AnceLayerTailGradArgs),
         (8, "ance_layer_tail16_workspace_bytes", "ance_layer_tail16_forward", "ance_layer_tail16_backward",
          _lib.AnceLayerTail16Args, _lib.AnceLayerTail16GradArgs))
_GELU = ((4, "ance_bias_gelu_workspace_bytes", "ance_bias_gelu_forward", "ance_bias_gelu_backward",
          _lib.AnceBiasGeluArgs, _lib.AnceBiasGeluGradArgs),
         (8, "ance_bias_gelu16_workspace_bytes", "ance_bias_gelu16_forward", "ance_bias_gelu16_backward",
          _lib.AnceBiasGelu16Args, _lib.AnceBiasGelu16GradArgs))


def _tail_forward(ctx, x, bias, residual, weight, beta, eps, dropout_p, training, half, want_half=False):
    """The forward of both tail Functions: x fp32, or with ``half`` fp16 / bf16 as it is (nothing is cast); residual fp32.  Returns
    (y, y16), y16 None unless ``want_half``."""
    L = _lib.lib()
    piece, ws_query, forward, _, Args, _ = _TAIL[half]
    shape, H = x.shape, x.shape[-1]
    (x, ld_x), (residual, ld_r) = _matrix(x, piece), _matrix(residual)
    bias, weight, beta = _vector(bias), _vector(weight), _vector(beta)
    n_rows = x.numel() // H
    if getattr(L, ws_query)(n_rows, H) == 0:
        raise _lib.AnceLibraryError("dropout_add_layer_norm: unsupported shape (rows %d, width %d)" % (n_rows, H))
    y = torch.empty(shape, dtype=torch.float32, device=x.device)
    y16 = torch.empty(shape, dtype=x.dtype, device=x.device) if want_half else None
    stats = torch.empty(_stats_floats(n_rows), dtype=torch.float32, device=x.device)
    drop = bool(training) and dropout_p > 0.0
    draw = dropout_state.draw(x.device) if drop else _NO_DRAW
    args = Args(x=x.data_ptr(), res=residual.data_ptr(), bias=_ptr(bias), gamma=weight.data_ptr(), beta=beta.data_ptr(), y=y.data_ptr(),
                ld_x=ld_x, ld_res=ld_r, ld_y=H, H=H, n_rows=n_rows, eps=float(eps), dropout_p=float(dropout_p),
                training=1 if drop else 0, seed=draw.seed, offset=draw.offset, d_workspace=stats.data_ptr(),
                workspace_bytes=stats.numel() * 4)
    if half:   # the fields only the 16-bit struct has
        args.y16, args.ld_y16, args.dtype = _ptr(y16), H, HALF_DTYPES[x.dtype]
    with torch.cuda.device(x.device):
        draw.launch(forward, ctypes.byref(args))
    ctx.save_for_backward(x, residual, bias, weight, stats)
    ctx.args, ctx.draw = args, draw
    ctx.shape = shape
    return y, y16


def _tail_backward(ctx, dy, dy16, half):
    """The backward of both tail Functions -> (dx, dbias, dres, dgamma, dbeta): dx in x's dtype, the rest fp32.  With ``half``, dy
    and dy16 may each be None (not both)."""
    L = _lib.lib()
    piece, ws_query, _, backward, Args, GradArgs = _TAIL[half]
    x, residual, bias, weight, stats = ctx.saved_tensors
    a = Args.from_buffer_copy(ctx.args)  # y, y16 and beta are not touched by the backward
    H, n_rows = a.H, a.n_rows
    ld_dy = ld_dy16 = 0
    if dy is not None:
        dy, ld_dy = _matrix(dy.to(torch.float32))
    if dy16 is not None:
        dy16, ld_dy16 = _matrix(dy16.to(x.dtype), piece)
    want_x, want_bias, want_res, want_w, want_b = ctx.needs_input_grad[:5]

    def out(want, shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=x.device) if want else None

    dx, dres = out(want_x, ctx.shape, x.dtype), out(want_res, ctx.shape)
    dbias, dgamma, dbeta = out(want_bias and bias is not None, (H,)), out(want_w, (H,)), out(want_b, (H,))
    # the saved state is the statistics alone; the backward's partial rows live only as long as this call
    ws_bytes = getattr(L, ws_query)(n_rows, H)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device)
    ws[:stats.numel()].copy_(stats)
    a.d_workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
    g = GradArgs(dy=_ptr(dy), dx=_ptr(dx), dres=_ptr(dres), dgamma=_ptr(dgamma), dbeta=_ptr(dbeta), dbias=_ptr(dbias), ld_dy=ld_dy,
                 ld_dx=H, ld_dres=H)
    if half:
        g.dy16, g.ld_dy16 = _ptr(dy16), ld_dy16
    with torch.cuda.device(x.device):
        ctx.draw.launch(backward, ctypes.byref(a), ctypes.byref(g))
    return dx, dbias, dres, dgamma, dbeta


def _gelu_forward(ctx, x, bias, half):
    """The forward of both GELU Functions: y has x's dtype, and the saved input is x itself."""
    L = _lib.lib()
    piece, ws_query, forward, _, Args, _ = _GELU[half]
    shape, N = x.shape, x.shape[-1]
    x, ld_x = _matrix(x, piece)
    bias = _vector(bias)
    n_rows = x.numel() // N
    if getattr(L, ws_query)(n_rows, N) == 0:
        raise _lib.AnceLibraryError("bias_gelu: unsupported shape (rows %d, width %d)" % (n_rows, N))
    y = torch.empty(shape, dtype=x.dtype, device=x.device)
    args = Args(x=x.data_ptr(), bias=bias.data_ptr(), y=y.data_ptr(), ld_x=ld_x, ld_y=N, N=N, n_rows=n_rows, d_workspace=None,
                workspace_bytes=0)
    if half:
        args.dtype = HALF_DTYPES[x.dtype]
    with torch.cuda.device(x.device):
        _lib.check(getattr(L, forward)(ctypes.byref(args), _lib.current_stream_ptr()), forward)
    ctx.save_for_backward(x, bias)
    ctx.args = args
    ctx.shape = shape
    return y


def _gelu_backward(ctx, dy, half):
    """The backward of both GELU Functions -> (dx, dbias): dx in x's dtype, dbias fp32."""
    L = _lib.lib()
    piece, ws_query, _, backward, Args, GradArgs = _GELU[half]
    x, bias = ctx.saved_tensors
    a = Args.from_buffer_copy(ctx.args)
    dy, ld_dy = _matrix(dy.to(x.dtype), piece)
    want_x, want_bias = ctx.needs_input_grad[:2]
    dx = torch.empty(ctx.shape, dtype=x.dtype, device=x.device) if want_x else None
    dbias = torch.empty(a.N, dtype=torch.float32, device=x.device) if want_bias else None
    ws_bytes = getattr(L, ws_query)(a.n_rows, a.N)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device)
    a.d_workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
    g = GradArgs(dy=dy.data_ptr(), dx=_ptr(dx), dbias=_ptr(dbias), ld_dy=ld_dy, ld_dx=a.N)
    with torch.cuda.device(x.device):
        _lib.check(getattr(L, backward)(ctypes.byref(a), ctypes.byref(g), _lib.current_stream_ptr()), backward)
    return dx, dbias


class _DropoutAddLayerNorm(torch.autograd.Function):
    @staticmethod
    @_custom_fwd
    def forward(ctx, x, bias, residual, weight, beta, eps, dropout_p, training):
        return _tail_forward(ctx, x, bias, residual, weight, beta, eps, dropout_p, training, False)[0]

    @staticmethod
    @_custom_bwd
    @once_differentiable
    def backward(ctx, dy):
        return _tail_backward(ctx, dy, None, False) + (None, None, None)


class _BiasGelu(torch.autograd.Function):
    @staticmethod
    @_custom_fwd
    def forward(ctx, x, bias):
        return _gelu_forward(ctx, x, bias, False)

    @staticmethod
    @_custom_bwd
    @once_differentiable
    def backward(ctx, dy):
        return _gelu_backward(ctx, dy, False)


class _DropoutAddLayerNormHalf(torch.autograd.Function):
    """_DropoutAddLayerNorm with a 16-bit x and an fp32 residual stream (csrc/layer_tail_half.hip): nothing is cast.  Returns y (fp32)
    or, with want_half, (y, y16); the backward takes whichever of their two gradients exist and sums them in registers."""

    @staticmethod
    @_custom_fwd_as_is
    def forward(ctx, x, bias, residual, weight, beta, eps, dropout_p, training, want_half):
        y, y16 = _tail_forward(ctx, x, bias, residual, weight, beta, eps, dropout_p, training, True, want_half)
        ctx.set_materialize_grads(False)   # a missing gradient stays None: the kernel reads only those that exist
        return (y, y16) if want_half else y

    @staticmethod
    @_custom_bwd
    @once_differentiable
    def backward(ctx, dy, dy16=None):
        if dy is None and dy16 is None:
            return (None,) * 9
        return _tail_backward(ctx, dy, dy16, True) + (None, None, None, None)


class _BiasGeluHalf(torch.autograd.Function):
    """_BiasGelu from 16 bits to 16 bits (csrc/layer_tail_half.hip): the saved input is the 16-bit x itself."""

    @staticmethod
    @_custom_fwd_as_is
    def forward(ctx, x, bias):
        return _gelu_forward(ctx, x, bias, True)

    @staticmethod
    @_custom_bwd
    @once_differentiable
    def backward(ctx, dy):
        return _gelu_backward(ctx, dy, True)


def _half_rows(x, what, widths):
    """precision="half": x as the 16-bit kernels take it.  fp16 / bf16 go in as they are; an fp32 x is cast to the autocast dtype
    under autocast (a differentiable cast, as autocast's own) and refused outside it."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _lib.AnceLibraryError("%s must be a CUDA(HIP) tensor" % what)
    if x.dtype == torch.float32 and torch.is_autocast_enabled():
        x = x.to(torch.get_autocast_dtype("cuda") if hasattr(torch, "get_autocast_dtype") else torch.get_autocast_gpu_dtype())
    if x.dtype not in HALF_DTYPES:
        raise _lib.AnceLibraryError("%s must have dtype torch.float16 or bfloat16 with precision=\"half\", got %s" % (what, x.dtype))
    if x.dim() < 2 or x.shape[-1] not in widths:
        raise _lib.AnceLibraryError("%s must be [.., W] with W in %r, got %r" % (what, widths, tuple(x.shape)))
    if x.numel() == 0:
        raise _lib.AnceLibraryError("empty input")
    return x


def _check_fp32(t, what):
    """precision="half": the residual stream and the parameters stay fp32, under autocast as well (nothing casts them)."""
    if t is not None and isinstance(t, torch.Tensor) and t.dtype != torch.float32:
        raise _lib.AnceLibraryError("%s must have dtype torch.float32 with precision=\"half\", got %s" % (what, t.dtype))


def dropout_add_layer_norm(x, bias, residual, weight, beta, eps, dropout_p=0.0, training=True, precision="fp32", return_half=False):
    """LayerNorm(dropout(x + bias) + residual) * weight + beta over the last dimension: x, residual [.., H] fp32 with H 768 or 1024
    (views with evenly spaced rows pass as they are, anything else is copied), bias [H] or None, weight, beta [H].  Returns y shaped
    like x; gradients for x, bias, residual, weight and beta.
    precision="half" (for ``torch.autocast``): x is fp16 or bf16 and goes in as it is -- the dense output without its bias -- while
    residual, the parameters and y stay fp32: the residual stream is never rounded to 16 bits.  An fp32 x is cast to the autocast
    dtype under autocast and refused outside it.  The gradient of x has x's dtype, every other gradient is fp32.
    ``return_half=True`` returns (y, y16): y16 is y rounded once to x's dtype in the same launch, for the Linears that read y; both
    are differentiable and the backward sums whichever of their gradients exist in registers."""
    half = _check_precision(precision)
    if not half and return_half:
        raise _lib.AnceLibraryError("return_half needs precision=\"half\"")
    if half:
        x = _half_rows(x, "x", TAIL_WIDTHS)
        for t, what in ((residual, "residual"), (bias, "bias"), (weight, "weight"), (beta, "beta")):
            _check_fp32(t, what)
    else:
        _check_rows(x, "x", TAIL_WIDTHS)
    _check_rows(residual, "residual", TAIL_WIDTHS)
    if residual.shape != x.shape or residual.device != x.device:
        raise _lib.AnceLibraryError("x and residual must be of one shape, on one device")
    H = x.shape[-1]
    _check_vector(bias, "bias", H, x, optional=True)
    _check_vector(weight, "weight", H, x)
    _check_vector(beta, "beta", H, x)
    if not 0.0 <= float(dropout_p) < 1.0:
        raise _lib.AnceLibraryError("dropout_p must be in [0, 1), got %r" % (dropout_p,))
    if not float(eps) > 0.0:
        raise _lib.AnceLibraryError("eps must be positive, got %r" % (eps,))
    if half:
        return _DropoutAddLayerNormHalf.apply(x, bias, residual, weight, beta, float(eps), float(dropout_p), bool(training),
                                              bool(return_half))
    return _DropoutAddLayerNorm.apply(x, bias, residual, weight, beta, float(eps), float(dropout_p), bool(training))


def bias_gelu(x, bias, precision="fp32"):
    """gelu(x + bias), the erf form, over [.., N] fp32 with N 3072 or 4096; gradients for x and bias.
    precision="half": x is fp16 or bf16 (an fp32 x is cast under autocast and refused outside it), bias fp32; y and the gradient of
    x have x's dtype, the arithmetic is fp32 with one rounding at the store, and the saved input is the 16-bit x."""
    if _check_precision(precision):
        x = _half_rows(x, "x", GELU_WIDTHS)
        _check_fp32(bias, "bias")
        _check_vector(bias, "bias", x.shape[-1], x)
        return _BiasGeluHalf.apply(x, bias)
    _check_rows(x, "x", GELU_WIDTHS)
    _check_vector(bias, "bias", x.shape[-1], x)
    return _BiasGelu.apply(x, bias)


class _ZeroGradient(torch.autograd.Function):
    """attention.self.key.bias as the key Linear reads it: the same values, and a gradient of exact zeros.  A bias on the keys adds
    q_i . b to every score of query row i, a constant along the row that softmax does not see -- with the pad mask and with dropout
    on the probabilities alike -- so the gradient IS zero; the column sum of dk that autograd would hand back is its rounding
    noise (measured 1e-7 against query.bias's 0.2, several times the eager expression's own noise: the core takes the row term of
    the softmax backward from ctx), and LAMB / Adam turn noise into steps of lr."""

    @staticmethod
    def forward(ctx, bias):
        return bias.view_as(bias)

    @staticmethod
    def backward(ctx, grad):
        return torch.zeros_like(grad)


class _Namespace(torch.nn.Module):
    """A module that only holds submodules: the names of transformers' BertLayer, so that its state dict loads as it is."""


def _all_rows(t):
    return t


def _first_of_padded(t):
    return t[:, 0]


class BertLayer(torch.nn.Module):
    """transformers' BertLayer (2.3.0 modeling_bert.py; RoBERTa's towers run the same class) for right-padded batches, with the same
    submodule and parameter names: attention.self.query / key / value, attention.output.dense / LayerNorm, intermediate.dense,
    output.dense / LayerNorm.  ``forward(hidden_states [B, L, H] fp32, lens [B])`` runs six F.linear calls (the three dense ones
    without their bias, which goes into the fused call behind them), attention_padded, two dropout_add_layer_norm and one bias_gelu.
    ``attention_precision="half"`` is for ``torch.autocast``: the fp16 / bf16 Linear outputs enter the attention core as they are and
    ctx goes into attention.output.dense without a cast (attention_padded, precision="half"); with fp32 hidden states outside autocast
    it raises.  With it alone the three row-wise seams stay fp32.
    ``precision="half"`` (implies ``attention_precision="half"``) runs the seams in 16 bits as well and keeps the residual stream in
    fp32: ``forward(hidden_states, lens, hidden_states_half=None, return_half=False)`` takes the fp32 hidden states (the residual)
    and, optionally, their 16-bit copy -- otherwise the layer makes that ONE cast itself; the three q / k / v Linears read it, the
    first tail returns (h, h16) and intermediate.dense reads h16, the GELU runs 16 bits to 16 bits, and the second tail returns the
    fp32 output, or with ``return_half=True`` (out, out16) for the next layer's ``hidden_states_half``: a stack of layers then runs
    with no activation cast after the first.  The parameters and their gradients stay fp32.
    attention.self.key.bias gets a gradient of exact zeros (it has none: softmax does not see a constant added to a row of
    scores), not the rounding noise of the column sum of dk.
    Pad rows are computed like any other in the three row-wise seams, as the reference does; the attention core writes zeros there
    (INTEGRATION.md 3i), so a pad row of the output is the LayerNorm tail of zeros, not the reference's value, and never reaches a
    loss.
    The four forms -- ``forward``, ``forward_first_rows``, ``forward_packed``, ``forward_first_rows_packed`` -- are their own checks
    in front of ONE forward text, ``_layer``."""

    def __init__(self, hidden_size, num_attention_heads, intermediate_size, layer_norm_eps=1e-12, hidden_dropout_prob=0.1,
                 attention_probs_dropout_prob=0.1, attention_precision="fp32", precision="fp32"):
        super().__init__()
        if attention_precision not in ("fp32", "half"):
            raise _lib.AnceLibraryError("BertLayer: attention_precision must be \"fp32\" or \"half\", got %r" % (attention_precision,))
        if precision not in ("fp32", "half"):
            raise _lib.AnceLibraryError("BertLayer: precision must be \"fp32\" or \"half\", got %r" % (precision,))
        self.precision = precision
        self.attention_precision = "half" if precision == "half" else attention_precision
        if hidden_size not in TAIL_WIDTHS or hidden_size != 64 * num_attention_heads or intermediate_size not in GELU_WIDTHS:
            raise _lib.AnceLibraryError("BertLayer: hidden_size must be 768 (12 heads) or 1024 (16 heads), intermediate_size 3072 or "
                                        "4096; got %r, %r heads, %r" % (hidden_size, num_attention_heads, intermediate_size))
        nn = torch.nn
        self.num_attention_heads, self.layer_norm_eps = num_attention_heads, float(layer_norm_eps)
        self.hidden_dropout_prob, self.attention_probs_dropout_prob = float(hidden_dropout_prob), float(attention_probs_dropout_prob)
        self.attention = _Namespace()
        self.attention.self = _Namespace()
        for name in ("query", "key", "value"):
            setattr(self.attention.self, name, nn.Linear(hidden_size, hidden_size))
        self.attention.output = _Namespace()
        self.attention.output.dense = nn.Linear(hidden_size, hidden_size)
        self.attention.output.LayerNorm = nn.LayerNorm(hidden_size, eps=layer_norm_eps)
        self.intermediate = _Namespace()
        self.intermediate.dense = nn.Linear(hidden_size, intermediate_size)
        self.output = _Namespace()
        self.output.dense = nn.Linear(intermediate_size, hidden_size)
        self.output.LayerNorm = nn.LayerNorm(hidden_size, eps=layer_norm_eps)

    def _projection_rows(self, hidden_states, hidden_states_half, return_half=False):
        """The checks of (hidden_states, hidden_states_half, return_half) that every form makes; returns the rows the projections
        read: hidden_states itself, or with precision="half" its 16-bit copy (the one given, or the layer's one activation cast)."""
        if self.precision != "half":
            if hidden_states_half is not None or return_half:
                raise _lib.AnceLibraryError("BertLayer: hidden_states_half and return_half need precision=\"half\"")
            return hidden_states
        if not isinstance(hidden_states, torch.Tensor) or hidden_states.dtype != torch.float32:
            raise _lib.AnceLibraryError("BertLayer(precision=\"half\"): hidden_states is the fp32 residual stream, got %s"
                                        % (getattr(hidden_states, "dtype", type(hidden_states)),))
        if hidden_states_half is None:   # the layer's one activation cast
            return _half_rows(hidden_states, "hidden_states", TAIL_WIDTHS)
        if hidden_states_half.dtype not in HALF_DTYPES or hidden_states_half.shape != hidden_states.shape:
            raise _lib.AnceLibraryError("hidden_states_half must be the fp16 / bf16 copy of hidden_states, got %s %r"
                                        % (hidden_states_half.dtype, tuple(hidden_states_half.shape)))
        return hidden_states_half

    def _check_packed(self, hidden_states, packed, what):
        if not isinstance(packed, PackedTokens):
            raise _lib.AnceLibraryError("BertLayer.%s: packed must be a PackedTokens (ance_amd.packing.pack_tokens)" % what)
        if not isinstance(hidden_states, torch.Tensor) or hidden_states.dim() != 2 or hidden_states.shape[0] != packed.rows:
            raise _lib.AnceLibraryError("BertLayer.%s: hidden_states must be [R, H] with the packed batch's R = %d rows" % (what, packed.rows))

    def _layer(self, x, residual, rows, attention, return_half=False):
        """The forward text of every form.  x: the rows the key and value projections read (``_projection_rows``); residual: the
        fp32 hidden states; rows: what the query projection and the seams run over -- all rows (identity) or the sequences' first
        rows (``t[:, 0]``, ``first_rows(t, packed)``), applied to x and to residual; attention(q, k, v): the core's call of the
        form.  Three draws of the dropout stream in training: attention, first tail, second tail."""
        F = torch.nn.functional
        att, eps, p = self.attention, self.layer_norm_eps, self.hidden_dropout_prob
        half = self.precision == "half"
        prec = dict(precision="half") if half else {}
        q = F.linear(rows(x), att.self.query.weight, att.self.query.bias)
        k = F.linear(x, att.self.key.weight, _ZeroGradient.apply(att.self.key.bias))
        v = F.linear(x, att.self.value.weight, att.self.value.bias)
        ctx = attention(q, k, v)
        ln = att.output.LayerNorm
        h = dropout_add_layer_norm(F.linear(ctx, att.output.dense.weight), att.output.dense.bias, rows(residual), ln.weight, ln.bias,
                                   eps, p, self.training, return_half=half, **prec)
        h, h_in = h if half else (h, h)   # half: (h, h16), and intermediate.dense reads the 16-bit copy
        t = bias_gelu(F.linear(h_in, self.intermediate.dense.weight), self.intermediate.dense.bias, **prec)
        ln = self.output.LayerNorm
        return dropout_add_layer_norm(F.linear(t, self.output.dense.weight), self.output.dense.bias, h, ln.weight, ln.bias, eps, p,
                                      self.training, return_half=return_half, **prec)

    def forward(self, hidden_states, lens, hidden_states_half=None, return_half=False):
        x = self._projection_rows(hidden_states, hidden_states_half, return_half)
        return self._layer(x, hidden_states, _all_rows, lambda q, k, v: attention_padded(
            q, k, v, lens, self.num_attention_heads, self.attention_probs_dropout_prob, self.training,
            precision=self.attention_precision), return_half)

    def forward_first_rows(self, hidden_states, lens, hidden_states_half=None):
        """``forward(...)[:, 0]`` -- [B, H] fp32 -- for a tower's LAST layer, of which only the first rows are read: the key and the
        value projections run over all rows, everything else over the B first rows.  q0 = the query Linear of hidden_states[:, 0],
        attention_first_row, then the three seams on B rows with the residual hidden_states[:, 0] as a strided view.  Three draws of
        the dropout stream in forward's order; the attention mask is forward's query row 0 bit for bit, the tails' masks are those
        of a B-row call (row b, not row b * L).  precision="half": the projections read hidden_states_half (or the layer's one cast)
        and the seams run as in forward."""
        if not isinstance(hidden_states, torch.Tensor) or hidden_states.dim() != 3:
            raise _lib.AnceLibraryError("BertLayer.forward_first_rows: hidden_states must be [B, L, H]")
        x = self._projection_rows(hidden_states, hidden_states_half)
        return self._layer(x, hidden_states, _first_of_padded, lambda q0, k, v: attention_first_row(
            q0, k, v, lens, self.num_attention_heads, self.attention_probs_dropout_prob, self.training,
            precision=self.attention_precision))

    def forward_packed(self, hidden_states, packed, hidden_states_half=None, return_half=False):
        """``forward`` over the R rows of a PackedTokens: hidden_states [R, H] fp32 -> [R, H] fp32 (precision="half": with
        ``hidden_states_half`` / ``return_half`` as in forward).  The statements are forward's with attention_packed in place of
        attention_padded: the Linears and the seams run over R rows instead of B * L.  The attention's dropout mask is forward's
        bit for bit; the tails' masks are those of an R-row call.  A slack row (one that no sequence covers) is computed like any
        other by the seams, from a zero context: finite, and never read by a kept sequence; its gradient is exactly zero."""
        self._check_packed(hidden_states, packed, "forward_packed")
        x = self._projection_rows(hidden_states, hidden_states_half, return_half)
        return self._layer(x, hidden_states, _all_rows, lambda q, k, v: attention_packed(
            q, k, v, packed.seq_off, packed.max_seq_len, self.num_attention_heads, self.attention_probs_dropout_prob, self.training,
            precision=self.attention_precision), return_half)

    def forward_first_rows_packed(self, hidden_states, packed, hidden_states_half=None):
        """``forward_first_rows`` over the R rows of a PackedTokens -> [B, H] fp32: ``first_rows`` in place of ``x[:, 0]`` and
        attention_first_row_packed in place of attention_first_row.  An empty sequence's row is the tails of a zero residual and a
        zero context; a DROPPED sequence's row is NaN (first_rows), which is how an overflow of the capacity reaches the loss."""
        self._check_packed(hidden_states, packed, "forward_first_rows_packed")
        x = self._projection_rows(hidden_states, hidden_states_half)
        return self._layer(x, hidden_states, lambda t: first_rows(t, packed), lambda q0, k, v: attention_first_row_packed(
            q0, k, v, packed.seq_off, packed.max_seq_len, self.num_attention_heads, self.attention_probs_dropout_prob, self.training,
            precision=self.attention_precision))


class _Names(object):
    """A plain holder of attributes (not an nn.Module: what it holds is registered elsewhere, under other names)."""

    def __init__(*args, **kw):   # no named first parameter: "self" is one of the attribute names (attention.self)
        args[0].__dict__.update(kw)


class SeedLayer(BertLayer):
    """fairseq's post-LayerNorm TransformerSentenceEncoderLayer -- the SEED-Encoder's -- under ITS submodule names: self_attn.q_proj /
    k_proj / v_proj / out_proj, self_attn_layer_norm, fc1, fc2, final_layer_norm, so that ``named_parameters()`` and
    ``state_dict()`` are the reference's.  The layer is BertLayer's in arithmetic (q scaled by 1/8, attention-probability dropout,
    dropout on the attention output and on fc2's output, erf-GELU, eps 1e-5; activation_dropout = 0), and the forward text IS
    BertLayer's: ``attention``, ``intermediate`` and ``output`` are plain holders that name the same eight modules the way BertLayer's
    methods read them, registered once, under fairseq's names.  self_attn.k_proj.bias gets attention.self.key.bias's exact-zero
    gradient."""

    def __init__(self, hidden_size, num_attention_heads, intermediate_size, layer_norm_eps=1e-5, dropout=0.1, attention_dropout=0.1,
                 precision="fp32"):
        torch.nn.Module.__init__(self)
        if precision not in ("fp32", "half"):
            raise _lib.AnceLibraryError("SeedLayer: precision must be \"fp32\" or \"half\", got %r" % (precision,))
        self.precision = self.attention_precision = precision
        if hidden_size not in TAIL_WIDTHS or hidden_size != 64 * num_attention_heads or intermediate_size not in GELU_WIDTHS:
            raise _lib.AnceLibraryError("SeedLayer: hidden_size must be 768 (12 heads) or 1024 (16 heads), intermediate_size 3072 or "
                                        "4096; got %r, %r heads, %r" % (hidden_size, num_attention_heads, intermediate_size))
        nn = torch.nn
        self.num_attention_heads, self.layer_norm_eps = num_attention_heads, float(layer_norm_eps)
        self.hidden_dropout_prob, self.attention_probs_dropout_prob = float(dropout), float(attention_dropout)
        self.self_attn = _Namespace()
        for name in ("k_proj", "v_proj", "q_proj", "out_proj"):   # the reference's order of registration
            setattr(self.self_attn, name, nn.Linear(hidden_size, hidden_size))
        self.self_attn_layer_norm = nn.LayerNorm(hidden_size, eps=layer_norm_eps)
        self.fc1 = nn.Linear(hidden_size, intermediate_size)
        self.fc2 = nn.Linear(intermediate_size, hidden_size)
        self.final_layer_norm = nn.LayerNorm(hidden_size, eps=layer_norm_eps)
        a = self.self_attn
        self.attention = _Names(output=_Names(dense=a.out_proj, LayerNorm=self.self_attn_layer_norm),
                                **{"self": _Names(query=a.q_proj, key=a.k_proj, value=a.v_proj)})
        self.intermediate = _Names(dense=self.fc1)
        self.output = _Names(dense=self.fc2, LayerNorm=self.final_layer_norm)
