"""The 16-bit BertLayer seams (ance_amd/layers.py precision="half" -> csrc/layer_tail_half.hip) on the GPU against the fp64
restatements of tests/layer_half_util.py on the SAME 16-bit-valued inputs, against the fp32 seams bit for bit, and the whole
BertLayer(precision="half") under torch.autocast against the fp32 BertLayer.

Bounds.  B32(t) = layer_tail_util.bound = max(4 x the eager fp32 expression's own distance from fp64 on the same inputs and the same
restated mask, 16 ulp32 of the fp64 tensor's largest magnitude): the fp32 seams' bound, which the fp32 outputs here (y, dres, dgamma,
dbeta, dbias) are held to.  A 16-bit output (y16, dx; the GELU's y and dx) is held, elementwise, to half a dtype ulp at the larger of
the two magnitudes plus B32 (layer_half_util.within16).  Every measured figure is printed before it is asserted."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import attention_train_util as A
import layer_half_util as HU
import layer_tail_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 0x5EED0123456789AB
ROWS = (1, 15, 16, 17, 63, 64, 65, 2085)   # 2085 = 130 x 16 + 5: more than eight partial rows per slice of the column-sum tree
FP32_NAMES = ("y", "dres", "dgamma", "dbeta", "dbias")


def _dev(x, dtype=None, grad=False):
    if x is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    if dtype is not None:
        t = t.to(dtype)
    return t.requires_grad_(True) if grad else t


def _np(t):
    return None if t is None else t.detach().float().cpu().numpy()


def _same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    v = torch.int32 if a.dtype == torch.float32 else torch.int16
    return bool(torch.equal(a.contiguous().view(v), b.contiguous().view(v)))


def _tail16(x, b, r, g, be, eps, dy, dy16, name, p=0.0, training=True, want_half=True):
    """The half tail and its backward on device tensors (dy fp32 and dy16 16-bit, each optional); the raw tensors."""
    from ance_amd.layers import dropout_add_layer_norm
    dt = HU.torch_dtype(name)
    tx = _dev(x, dt, True)
    tb, tr, tg, tbe = (_dev(t, None, True) for t in (b, r, g, be))
    out = dropout_add_layer_norm(tx, tb, tr, tg, tbe, eps, p, training, precision="half", return_half=want_half)
    y, y16 = out if want_half else (out, None)
    assert y.dtype == torch.float32 and (y16 is None or y16.dtype == dt)
    outs, grads = [], []
    if dy is not None:
        outs.append(y)
        grads.append(_dev(dy))
    if dy16 is not None:
        outs.append(y16)
        grads.append(_dev(dy16, dt))
    torch.autograd.backward(outs, grads)
    assert tx.grad.dtype == dt and all(t.grad.dtype == torch.float32 for t in (tr, tg, tbe))
    return dict(y=y.detach(), y16=None if y16 is None else y16.detach(), dx=tx.grad, dres=tr.grad, dgamma=tg.grad, dbeta=tbe.grad,
                dbias=tb.grad if tb is not None else None)


def _tail32(x, b, r, g, be, eps, dy, p=0.0, training=True):
    """The fp32 tail on the same (16-bit-valued) x as fp32."""
    from ance_amd.layers import dropout_add_layer_norm
    tx, tb, tr, tg, tbe = (_dev(t, None, True) for t in (x, b, r, g, be))
    y = dropout_add_layer_norm(tx, tb, tr, tg, tbe, eps, p, training)
    y.backward(dy)
    return dict(y=y.detach(), dx=tx.grad, dres=tr.grad, dgamma=tg.grad, dbeta=tbe.grad, dbias=tb.grad if tb is not None else None)


def _check_tail(tag, got, want, ref, name):
    """got: device tensors of _tail16; want: tail16_fp64; ref: the eager fp32 expression's distances."""
    bad = []
    for n in FP32_NAMES:
        if want[n] is None:
            continue
        d = float(np.abs(_np(got[n]).astype(np.float64) - want[n]).max())
        b = U.bound(ref[n], np.abs(want[n]).max())
        print("%-46s %-6s max|delta| %.3e  reference %.3e  ratio %6.2f  bound %.3e" % (tag, n, d, ref[n], d / max(ref[n], 1e-300), b))
        if not d <= b:
            bad.append((n, d, b))
    for n16, n in (("y16", "y"), ("dx", "dx")):
        if got[n16] is None:
            continue
        b32 = U.bound(ref[n], np.abs(want[n]).max())
        ok, worst = HU.within16(_np(got[n16]), want[n], b32, name)
        print("%-46s %-6s (%s) worst |delta| / (ulp16 / 2 + B32) %.3f  B32 %.3e" % (tag, n16, name, worst, b32))
        if not ok:
            bad.append((n16, worst))
    assert not bad, (tag, bad)


@functools.lru_cache(maxsize=None)
def _tail_case(tag, n_rows, H, p, eps, name, offset=0, bias=True):
    """Seeded inputs rounded to the dtype (x and dy16; the rest stays fp32), the mask of (SEED, offset), the fp64 restatement with
    g = dy + dy16 and the eager fp32 expression's distances on the same inputs: once, on the CPU."""
    x, b, r, g, be, dy = U.tail_inputs(tag, n_rows, H, bias=bias)
    x, dy16 = HU.rounded(x, name), HU.rounded(U.det_normal(53, tag + ".dy16", (n_rows, H), 0.1), name)
    keep = U.tail_keep_mask(p, SEED, offset, n_rows, H) if p > 0 else None
    want = HU.tail16_fp64(x, b, r, g, be, eps, dy, dy16, name, keep, p)
    ref = U.distances(U.tail_eager_fp32(x, b, r, g, be, eps, dy + dy16, keep, p), want, U.TAIL_NAMES)
    return (x, b, r, g, be, dy, dy16), want, ref


@functools.lru_cache(maxsize=None)
def _gelu_case(tag, n_rows, N, name):
    x, b, dy = U.gelu_inputs(tag, n_rows, N)
    x, dy = HU.rounded(x, name), HU.rounded(dy, name)
    want = HU.gelu16_fp64(x, b, dy, name)
    return (x, b, dy), want, U.distances(U.gelu_eager_fp32(x, b, dy), want, U.GELU_NAMES)


def _gelu16(x, b, dy, name):
    from ance_amd.layers import bias_gelu
    dt = HU.torch_dtype(name)
    tx, tb = _dev(x, dt, True), _dev(b, None, True)
    y = bias_gelu(tx, tb, precision="half")
    assert y.dtype == dt
    y.backward(_dev(dy, dt))
    assert tx.grad.dtype == dt and tb.grad.dtype == torch.float32
    return dict(y=y.detach(), dx=tx.grad, dbias=tb.grad)


def _check_gelu(tag, got, want, ref, name, names=("y", "dx", "dbias")):
    bad = []
    for n in names:
        b32 = U.bound(ref[n], np.abs(want[n]).max())
        if n == "dbias":
            d = float(np.abs(_np(got[n]).astype(np.float64) - want[n]).max())
            print("%-46s %-6s max|delta| %.3e  reference %.3e  bound %.3e" % (tag, n, d, ref[n], b32))
            ok = d <= b32
        else:
            ok, worst = HU.within16(_np(got[n]), want[n], b32, name)
            print("%-46s %-6s (%s) worst |delta| / (ulp16 / 2 + B32) %.3f  B32 %.3e" % (tag, n, name, worst, b32))
        if not ok:
            bad.append(n)
    assert not bad, (tag, bad)


# ------------------------------------------------------------------------------------------------------------------------ row sweep
@pytest.mark.parametrize("name", HU.DTYPES)
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("H", [768, 1024])
def test_tail_row_sweep_bounds_and_fp32_bits(H, p, name):
    """Per row count: with both gradients, every output within its bound, y16 == y.to(dtype) bit for bit, and y, dres, dgamma, dbeta,
    dbias the fp32 tail's bits on x.float() and dy + dy16.float(), dx that dx rounded; then the same bits with dy alone and with
    dy16 alone."""
    from ance_amd import attention as T
    dt = HU.torch_dtype(name)
    for n_rows in ROWS:
        inp, want, ref = _tail_case("half.sweep.%d" % H, n_rows, H, p, 1e-5, name)
        x, b, r, g, be, dy, dy16 = inp
        tag = "tail16 %s H %d p %.1f rows %d" % (name, H, p, n_rows)
        for mode in ("both", "dy", "dy16"):
            T.manual_seed(SEED)   # offset 0
            got = _tail16(x, b, r, g, be, 1e-5, dy if mode != "dy16" else None, dy16 if mode != "dy" else None, name, p)
            if mode == "both":
                _check_tail(tag, got, want, ref, name)
            assert _same_bits(got["y16"], got["y"].to(dt)), (tag, mode, "y16 is y rounded once")
            total = {"both": _dev(dy) + _dev(dy16, dt).float(), "dy": _dev(dy), "dy16": _dev(dy16, dt).float()}[mode]
            T.manual_seed(SEED)
            base = _tail32(x, b, r, g, be, 1e-5, total, p)
            for n in FP32_NAMES:
                assert _same_bits(got[n], base[n]), (tag, mode, n, "the fp32 tail's bits")
            assert _same_bits(got["dx"], base["dx"].to(dt)), (tag, mode, "dx is the fp32 tail's dx rounded")


@pytest.mark.parametrize("name", HU.DTYPES)
@pytest.mark.parametrize("N", [3072, 4096])
def test_gelu_row_sweep(N, name):
    for n_rows in ROWS:
        inp, want, ref = _gelu_case("half.sweep.%d" % N, n_rows, N, name)
        _check_gelu("gelu16 %s N %d rows %d" % (name, N, n_rows), _gelu16(*inp, name), want, ref, name)


# ------------------------------------------------------------------------------------------------------------------------ golden
@pytest.mark.parametrize("name", HU.DTYPES)
@pytest.mark.parametrize("case", U.GOLDEN_CASES)
def test_golden_seams_rounded_to_the_dtype(golden_dir, case, name):
    """Both towers' own tensors at the three seams, x (and the GELU's dy) rounded to the dtype, eval mode."""
    m, seams = U.load_golden(golden_dir, case)
    for seam in U.SEAMS:
        t = seams[seam]
        if seam in U.TAILS:
            x = HU.rounded(t["x"], name)
            want = HU.tail16_fp64(x, t["bias"], t["res"], t["gamma"], t["beta"], m["eps"], t["dy"], None, name)
            ref = U.distances(U.tail_eager_fp32(x, t["bias"], t["res"], t["gamma"], t["beta"], m["eps"], t["dy"]), want, U.TAIL_NAMES)
            got = _tail16(x, t["bias"], t["res"], t["gamma"], t["beta"], m["eps"], t["dy"], None, name, 0.1, False)
            _check_tail("golden %s %s" % (case, seam), got, want, ref, name)
        else:
            x, dy = HU.rounded(t["x"], name), HU.rounded(t["dy"], name)
            want = HU.gelu16_fp64(x, t["bias"], dy, name)
            ref = U.distances(U.gelu_eager_fp32(x, t["bias"], dy), want, U.GELU_NAMES)
            _check_gelu("golden %s %s" % (case, seam), _gelu16(x, t["bias"], dy, name), want, ref, name)


# ------------------------------------------------------------------------------------------------------------------------ cases
@pytest.mark.parametrize("name", HU.DTYPES)
def test_strided_x_gives_the_contiguous_bits(name):
    from ance_amd import attention as T
    from ance_amd.layers import bias_gelu, dropout_add_layer_norm
    dt = HU.torch_dtype(name)
    H, n = 768, 37
    (x, b, r, g, be, dy, dy16), _, _ = _tail_case("half.strides", n, H, 0.5, 1e-5, name)
    res = []
    for form in ("contiguous", "a column slice of a wider buffer"):
        if form == "contiguous":
            tx = _dev(x, dt, True)
        else:
            wide = _dev(np.concatenate([np.full_like(x, np.nan), x, np.full_like(x, np.nan)], axis=1), dt, True)
            tx = wide[:, H:2 * H]
            assert tx.stride(0) == 3 * H and not tx.is_contiguous()
        tb, tr, tg, tbe = (_dev(t, None, True) for t in (b, r, g, be))
        T.manual_seed(SEED)
        y, y16 = dropout_add_layer_norm(tx, tb, tr, tg, tbe, 1e-5, 0.5, True, precision="half", return_half=True)
        grads = torch.autograd.grad([y, y16], [tx, tr, tb, tg, tbe], [_dev(dy), _dev(dy16, dt)])
        res.append([y.detach(), y16.detach()] + list(grads))
    for a, c in zip(*res):
        assert _same_bits(a, c)
    (gx, gb, gdy), _, _ = _gelu_case("half.strides", n, 3072, name)
    wide = _dev(np.concatenate([gx, np.full_like(gx, np.nan)], axis=1), dt, True)
    out = []
    for tx in (_dev(gx, dt, True), wide[:, :3072]):
        tb = _dev(gb, None, True)
        y = bias_gelu(tx, tb, precision="half")
        out.append([y.detach()] + list(torch.autograd.grad(y, [tx, tb], _dev(gdy, dt))))
    for a, c in zip(*out):
        assert _same_bits(a, c)


@pytest.mark.parametrize("name", HU.DTYPES)
def test_hard_rows_no_bias_and_no_y16(name):
    dt = HU.torch_dtype(name)
    H, n, eps = 768, 21, 1e-5
    x, b, r, g, be, dy = U.tail_inputs("half.hard", n, H)
    dy16 = HU.rounded(U.det_normal(53, "half.hard.dy16", (n, H), 0.1), name)

    def both(tag, x, b, r, g, be, dy, dy16, want_half=True):
        x = HU.rounded(x, name)
        want = HU.tail16_fp64(x, b, r, g, be, eps, dy, dy16, name)
        total = (dy if dy is not None else 0) + (dy16 if dy16 is not None else 0)
        ref = U.distances(U.tail_eager_fp32(x, b, r, g, be, eps, np.asarray(total, np.float32)), want, U.TAIL_NAMES)
        got = _tail16(x, b, r, g, be, eps, dy, dy16, name, want_half=want_half)
        _check_tail("%s %s" % (tag, name), got, want, ref, name)
        return got

    # mean 100, spread 0.01, carried by x (what survives the dtype's rounding of it) and by the fp32 residual
    both("mean 100 spread 0.01 in x", (100.0 + 0.01 * x).astype(np.float32), b * np.float32(0.01), np.zeros_like(r), g, be, dy, dy16)
    both("mean 100 spread 0.01 in res", 0.01 * x, b * np.float32(0.01), (100.0 + 0.01 * r).astype(np.float32), g, be, dy, dy16)
    # constant rows (short mantissas: exact in both dtypes and in every partial sum), bias = res = 0: y is beta bit for bit
    const = (np.arange(n, dtype=np.float32)[:, None] - 7.0) * np.float32(0.375) + np.zeros((n, H), np.float32)
    assert np.array_equal(HU.rounded(const, name), const)
    for bias in (np.zeros(H, np.float32), None):
        got = both("constant rows", const, bias, np.zeros_like(r), g, be, dy, dy16)
        want_y = _dev(np.ascontiguousarray(np.broadcast_to(be, (n, H))))
        assert _same_bits(got["y"], want_y), "y must equal beta bit for bit"
        assert _same_bits(got["y16"], want_y.to(dt)) and bool((got["dgamma"] == 0).all())
    # no bias: the kernel runs and returns no dbias
    got = both("bias None", x, None, r, g, be, dy, dy16)
    assert got["dbias"] is None
    # y16 not requested: the kernel runs without it, the other outputs keep their bits
    with_y16 = both("with y16", x, b, r, g, be, dy, None)
    without = both("y16 not requested", x, b, r, g, be, dy, None, want_half=False)
    assert without["y16"] is None
    for k in ("y", "dx", "dres", "dgamma", "dbeta", "dbias"):
        assert _same_bits(with_y16[k], without[k]), k


@pytest.mark.parametrize("name", HU.DTYPES)
def test_gelu_range(name):
    """u at +-0, +-1e-4, +-1, +-5, +-10, +-40 (rounded to the dtype): one column block of 256 per value, rows 1 .. 3 the values times
    (1 + k / 1024); finite outputs, each block within its own bound."""
    vals = [0.0, -0.0, 1e-4, -1e-4, 1.0, -1.0, 5.0, -5.0, 10.0, -10.0, 40.0, -40.0]
    N = 256 * len(vals)
    u = np.repeat(np.asarray(vals, np.float32), 256)[None, :] * np.ones((4, 1), np.float32)
    u[1:] *= (1.0 + np.arange(3 * N, dtype=np.float32).reshape(3, N) % 768 / 1024.0)
    x, b, dy = HU.rounded(u, name), np.zeros(N, np.float32), np.ones((4, N), np.float32)
    want, eager, got = HU.gelu16_fp64(x, b, dy, name), U.gelu_eager_fp32(x, b, dy), _gelu16(x, b, dy, name)
    for n in U.GELU_NAMES:
        assert bool(torch.isfinite(got[n]).all()), n
    for i, v in enumerate(vals):
        c = slice(256 * i, 256 * i + 256)
        blk = lambda d: {n: d[n][:, c] for n in ("y", "dx")}   # noqa: E731
        _check_gelu("gelu16 u = %g" % v, blk(got), blk(want), U.distances(blk(eager), blk(want), ("y", "dx")), name, ("y", "dx"))
    big, small = slice(256 * 10, 256 * 11), slice(256 * 11, 256 * 12)
    assert np.array_equal(_np(got["y"])[:, big], x[:, big]) and np.all(_np(got["dx"])[:, big] == 1.0)   # exactly u, the gradient 1
    assert np.all(_np(got["y"])[:, small] == 0.0) and np.all(_np(got["dx"])[:, small] == 0.0)
    _check_gelu("gelu16 range", got, want, U.distances(eager, want, ("dbias",)), name, ("dbias",))


def test_fp16_dx_overflow_arrives_as_inf_and_sets_found_inf():
    """A dx beyond 65504 is stored as +-inf, never clamped, so a GradScaler sees it: found_inf is 1 after unscale_."""
    from ance_amd.layers import dropout_add_layer_norm
    H, n = 768, 33
    x, b, r, g, be, dy = U.tail_inputs("half.overflow", n, H)
    x = HU.rounded(x, "fp16")
    big = (dy * np.float32(2e6)).astype(np.float32)   # dz is about rstd x dy: well past the fp16 range, and partly inside it
    got = _tail16(x, b, r, g, be, 1e-5, big, None, "fp16")
    base = _tail32(x, b, r, g, be, 1e-5, _dev(big))
    over = base["dx"].abs() >= 65520.0   # the rounding boundary between 65504 and inf
    assert bool(over.any()) and not bool(over.all())
    assert bool(torch.equal(torch.isinf(got["dx"]), over)) and bool((got["dx"][over].sign() == base["dx"][over].sign()).all())
    assert _same_bits(got["dx"], base["dx"].half()) and bool(torch.isfinite(got["dres"]).all())
    # through a Linear under autocast, as the trainers run it
    lin = torch.nn.Linear(H, H).to(DEV)
    opt = torch.optim.SGD(lin.parameters(), lr=0.1)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16)
    tr, tg, tbe = _dev(r), _dev(g), _dev(be)
    with torch.autocast("cuda", dtype=torch.float16):
        dense = torch.nn.functional.linear(_dev(x), lin.weight)
        assert dense.dtype == torch.float16
        y = dropout_add_layer_norm(dense, lin.bias, tr, tg, tbe, 1e-5, precision="half")
    scaler.scale((y * _dev(dy) * 100.0).sum()).backward()
    scaler.unscale_(opt)
    found = sum(float(v.item()) for v in scaler._per_optimizer_states[id(opt)]["found_inf_per_device"].values())
    assert found == 1.0 and not bool(torch.isfinite(lin.weight.grad).all())


# ------------------------------------------------------------------------------------------------------------------------ C ABI
def test_c_abi_writes_only_its_window():
    """Through ctypes, every output inside sentinel guard regions at row strides above the width (16-bit rows: multiples of 8): no
    guard element changes, and the windows hold the Python path's bits."""
    from ance_amd import _lib
    L_ = _lib.lib()
    st = _lib.current_stream_ptr()
    n, H, p, G = 37, 768, 0.5, 3
    (x, b, r, g, be, dy, dy16), want, ref = _tail_case("half.strides", n, H, p, 1e-5, "bf16", 3)
    dt = torch.bfloat16

    def guarded(ld, dtype, src=None):
        sent = torch.full((n + 2 * G, ld), float("nan"), dtype=dtype, device=DEV)
        if src is not None:
            sent[G:G + n, :H] = src
        return sent

    def intact(buf):
        return bool(torch.isnan(buf[:G]).all() and torch.isnan(buf[G + n:]).all() and torch.isnan(buf[:, H:]).all())

    bx, br = guarded(H + 16, dt, _dev(x, dt)), guarded(H + 4, torch.float32, _dev(r))
    bdy, bdy16 = guarded(H + 8, torch.float32, _dev(dy)), guarded(H + 24, dt, _dev(dy16, dt))
    by, by16, bdx, bdres = guarded(H + 8, torch.float32), guarded(H + 8, dt), guarded(H + 40, dt), guarded(H + 4, torch.float32)
    vec = [_dev(t) for t in (b, g, be)]
    col = torch.full((3, H + 64), float("nan"), dtype=torch.float32, device=DEV)
    ws_bytes = L_.ance_layer_tail16_workspace_bytes(n, H)
    ws = torch.full((ws_bytes // 4 + 64,), float("nan"), dtype=torch.float32, device=DEV)
    a = _lib.AnceLayerTail16Args(x=bx[G:].data_ptr(), res=br[G:].data_ptr(), bias=vec[0].data_ptr(), gamma=vec[1].data_ptr(),
                                 beta=vec[2].data_ptr(), y=by[G:].data_ptr(), y16=by16[G:].data_ptr(), ld_x=H + 16, ld_res=H + 4,
                                 ld_y=H + 8, ld_y16=H + 8, H=H, n_rows=n, dtype=_lib.ANCE_DTYPE_BF16, eps=1e-5, dropout_p=p, training=1,
                                 seed=SEED, offset=3, d_workspace=ws.data_ptr(), workspace_bytes=ws_bytes)
    gr = _lib.AnceLayerTail16GradArgs(dy=bdy[G:].data_ptr(), dy16=bdy16[G:].data_ptr(), dx=bdx[G:].data_ptr(), dres=bdres[G:].data_ptr(),
                                      dgamma=col[0].data_ptr(), dbeta=col[1].data_ptr(), dbias=col[2].data_ptr(), ld_dy=H + 8,
                                      ld_dy16=H + 24, ld_dx=H + 40, ld_dres=H + 4)
    _lib.check(L_.ance_layer_tail16_forward(ctypes.byref(a), st), "forward")
    _lib.check(L_.ance_layer_tail16_backward(ctypes.byref(a), ctypes.byref(gr), st), "backward")
    torch.cuda.synchronize()
    for nm, buf in (("y", by), ("y16", by16), ("dx", bdx), ("dres", bdres)):
        assert intact(buf), nm
    assert bool(torch.isnan(col[:, H:]).all()) and bool(torch.isnan(ws[ws_bytes // 4:]).all())
    got = dict(y=by[G:G + n, :H], y16=by16[G:G + n, :H], dx=bdx[G:G + n, :H], dres=bdres[G:G + n, :H], dgamma=col[0, :H], dbeta=col[1, :H],
               dbias=col[2, :H])
    _check_tail("C ABI tail16, strided", got, want, ref, "bf16")
    # a 16-bit row stride that is a multiple of 4 but not of 8 is refused, on real buffers, and nothing is written
    by.fill_(float("nan"))
    a.ld_x = H + 4
    assert L_.ance_layer_tail16_forward(ctypes.byref(a), st) == -1 and b"stride" in L_.ance_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(by).all())


# ------------------------------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("name", HU.DTYPES)
def test_deterministic_capturable_and_never_synchronises(name):
    from ance_amd import attention as T
    from ance_amd.layers import bias_gelu, dropout_add_layer_norm
    dt = HU.torch_dtype(name)
    H, N, n = 768, 3072, 70
    (x, b, r, g, be, dy, dy16), _, _ = _tail_case("half.capture", n, H, 0.1, 1e-5, name)
    (gx, gb, gdy), _, _ = _gelu_case("half.capture", n, N, name)
    tin = [_dev(x, dt)] + [_dev(t) for t in (b, r, g, be, dy)] + [_dev(dy16, dt), _dev(gx, dt), _dev(gb), _dev(gdy, dt)]

    def step(p):
        tx, tb, tr, tg, tbe = (t.clone().requires_grad_(True) for t in tin[:5])
        y, y16 = dropout_add_layer_norm(tx, tb, tr, tg, tbe, 1e-5, p, True, precision="half", return_half=True)
        torch.autograd.backward([y, y16], [tin[5], tin[6]])
        ux, ub = (t.clone().requires_grad_(True) for t in tin[7:9])
        z = bias_gelu(ux, ub, precision="half")
        z.backward(tin[9])
        return [y.detach(), y16.detach(), tx.grad, tb.grad, tr.grad, tg.grad, tbe.grad, z.detach(), ux.grad, ub.grad]

    for p in (0.0, 0.1):
        T.manual_seed(5)
        e1 = [t.clone() for t in step(p)]
        T.manual_seed(5)
        e2 = [t.clone() for t in step(p)]
        torch.cuda.synchronize()
        for a, c in zip(e1, e2):
            assert _same_bits(a, c)
        prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")  # any synchronising torch call raises
        try:
            step(p)
        finally:
            torch.cuda.set_sync_debug_mode(prev)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step(p)  # warm-up on the side stream, as torch's capture recipe asks
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        T.manual_seed(5)   # the captured launch bakes in (seed, offset 0): every replay draws the mask of e1
        with torch.cuda.graph(graph):
            outs = step(p)
        for _ in range(2):
            for t in outs:
                t.zero_()
            graph.replay()
            torch.cuda.synchronize()
            for a, c in zip(e1, outs):
                assert _same_bits(a, c)


def test_fp32_precision_keyword_is_the_default_path():
    """precision="fp32" spelled out runs the fp32 kernels: the default call's bits."""
    from ance_amd import attention as T
    from ance_amd.layers import bias_gelu, dropout_add_layer_norm
    (x, b, r, g, be, dy, _), _, _ = _tail_case("half.default", 19, 768, 0.1, 1e-5, "fp16")
    res = []
    for kw in (dict(), dict(precision="fp32")):
        T.manual_seed(SEED)
        tx, tb, tr, tg, tbe = (_dev(t, None, True) for t in (x, b, r, g, be))
        y = dropout_add_layer_norm(tx, tb, tr, tg, tbe, 1e-5, 0.1, True, **kw)
        y.backward(_dev(dy))
        res.append([y.detach(), tx.grad, tb.grad, tr.grad, tg.grad, tbe.grad])
    for a, c in zip(*res):
        assert a.dtype == torch.float32 and _same_bits(a, c)
    (gx, gb, _), _, _ = _gelu_case("half.default", 5, 3072, "fp16")
    assert _same_bits(bias_gelu(_dev(gx), _dev(gb)), bias_gelu(_dev(gx), _dev(gb), precision="fp32"))


# ------------------------------------------------------------------------------------------------------------------------ BertLayer
def _layer(hidden, heads, inter, eps, sd, p=0.0, **kw):
    from ance_amd.layers import BertLayer
    layer = BertLayer(hidden, heads, inter, eps, p, p, **kw).to(DEV)
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return layer


@pytest.mark.parametrize("dt", HU.DTYPES)
@pytest.mark.parametrize("lens,hidden,heads,inter", [((40, 9), 768, 12, 3072), ((17,), 1024, 16, 4096)])
def test_bert_layer_half_under_autocast(lens, hidden, heads, inter, dt):
    """BertLayer(precision="half") under torch.autocast: out, dhs and every parameter gradient within max(4 x D, 16 ulp32 of the
    tensor's largest magnitude) of the fp32 BertLayer (outside autocast) on the same weights, D = |eager autocast layer - the fp32
    BertLayer| per tensor (the floor: D is exactly 0 for output.LayerNorm.bias).  A spy on the seam functions sees 16-bit x going in,
    and no fp32 tensor of the intermediate width is saved for the backward.  The ratios are printed."""
    from ance_amd import layers as Lm
    dtype, eps = HU.torch_dtype(dt), 1e-5
    B, L = len(lens), max(lens)
    sd = U.layer_weights(hidden, inter)
    hs = U.det_normal(3, "half.hs.%d" % hidden, (B, L, hidden), 1.0)
    rows_np = A._valid(np.asarray(lens), L)
    dout = np.where(rows_np[:, :, None], U.det_normal(3, "half.dout.%d" % hidden, (B, L, hidden), 0.1), np.float32(0))
    rows, tlens, tdout = _dev(rows_np), _dev(np.asarray(lens, np.int32)), _dev(dout)

    def run_layer(autocast, **kw):
        layer = _layer(hidden, heads, inter, eps, sd, **kw)
        ths = _dev(hs, None, True)
        with torch.autocast("cuda", dtype=dtype, enabled=autocast):
            out = layer(ths, tlens)
        assert out.dtype == torch.float32
        out.backward(tdout)
        res = {k: _np(p.grad) for k, p in layer.named_parameters()}
        assert all(p.grad.dtype == torch.float32 for p in layer.parameters()) and ths.grad.dtype == torch.float32
        res["out"], res["dhs"] = (np.where(rows_np[:, :, None], _np(t), 0.0) for t in (out, ths.grad))
        return res

    seen, saved = [], []
    real_tail, real_gelu = Lm.dropout_add_layer_norm, Lm.bias_gelu

    def spy_tail(x, bias, residual, *a, **kw):
        seen.append(("tail", x.dtype, residual.dtype, kw.get("precision")))
        return real_tail(x, bias, residual, *a, **kw)

    def spy_gelu(x, bias, **kw):
        y = real_gelu(x, bias, **kw)
        seen.append(("gelu", x.dtype, y.dtype, kw.get("precision")))
        return y

    def pack(t):
        saved.append((tuple(t.shape), t.dtype))
        return t

    Lm.dropout_add_layer_norm, Lm.bias_gelu = spy_tail, spy_gelu
    try:
        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            got = run_layer(True, precision="half")
    finally:
        Lm.dropout_add_layer_norm, Lm.bias_gelu = real_tail, real_gelu
    assert seen == [("tail", dtype, torch.float32, "half"), ("gelu", dtype, dtype, "half"), ("tail", dtype, torch.float32, "half")], seen
    wide = [s for s in saved if s[0] and s[0][-1] == inter and int(np.prod(s[0])) == B * L * inter]
    assert wide and all(d == dtype for _, d in wide), wide   # the 3072-wide activations are saved, in 16 bits only
    base = run_layer(False)
    W = {k: _dev(v, None, True) for k, v in sd.items()}
    ths = _dev(hs, None, True)
    with torch.autocast("cuda", dtype=dtype):
        out = HU.eager_layer(ths, rows, W, heads, eps)
    out.float().backward(tdout)
    eager = {k: _np(w.grad) for k, w in W.items()}
    eager["out"], eager["dhs"] = (np.where(rows_np[:, :, None], _np(t), 0.0) for t in (out, ths.grad))
    bad, worst = [], 0.0
    for n in sorted(base):
        D = float(np.abs(eager[n].astype(np.float64) - base[n]).max())
        d = float(np.abs(got[n].astype(np.float64) - base[n]).max())
        bound = max(4.0 * D, 16.0 * A.ulp32(np.abs(base[n]).max()))
        if D > 0:
            worst = max(worst, d / D)
        print("BertLayer precision=half %s H %d %-36s |half - fp32| %.3e  D = |eager autocast - fp32| %.3e  ratio %5.2f  bound %.3e"
              % (dt, hidden, n, d, D, d / D if D > 0 else float("nan"), bound))
        if not d <= bound:
            bad.append((n, d, D, bound))
    print("BertLayer precision=half %s H %d largest ratio %.2f" % (dt, hidden, worst))
    assert not bad, bad


@pytest.mark.parametrize("dt", HU.DTYPES)
def test_two_layers_chained_through_the_16_bit_copy(dt):
    """return_half / hidden_states_half hand the second layer the first one's y16: the bits of the same two layers each making its
    own cast, forward and backward."""
    dtype, eps = HU.torch_dtype(dt), 1e-5
    hidden, heads, inter, lens = 768, 12, 3072, (40, 9)
    sd1, sd2 = U.layer_weights(hidden, inter), U.layer_weights(hidden, inter, seed=71)
    hs = U.det_normal(3, "half.hs.%d" % hidden, (2, 40, hidden), 1.0)
    tdout, tlens = _dev(U.det_normal(3, "half.dout.%d" % hidden, (2, 40, hidden), 0.1)), _dev(np.asarray(lens, np.int32))
    res = []
    for chained in (True, False):
        l1, l2 = _layer(hidden, heads, inter, eps, sd1, precision="half"), _layer(hidden, heads, inter, eps, sd2, precision="half")
        ths = _dev(hs, None, True)
        with torch.autocast("cuda", dtype=dtype):
            if chained:
                mid, mid16 = l1(ths, tlens, return_half=True)
                assert mid.dtype == torch.float32 and mid16.dtype == dtype
                out = l2(mid, tlens, hidden_states_half=mid16)
            else:
                out = l2(l1(ths, tlens), tlens)
        out.backward(tdout)
        res.append([out.detach(), ths.grad] + [p.grad for p in list(l1.parameters()) + list(l2.parameters())])
    for i, (a, c) in enumerate(zip(*res)):
        assert _same_bits(a, c), i


def test_peak_memory_is_below_the_half_attention_layer():
    """Forward + backward at 4 x 128 rows under autocast: no fp32 copy of the intermediate activation, 16-bit saved inputs."""
    hidden, heads, inter, eps = 768, 12, 3072, 1e-5
    sd = U.layer_weights(hidden, inter)
    hs, tdout = _dev(U.det_normal(3, "half.mem.hs", (4, 128, hidden), 1.0)), _dev(U.det_normal(3, "half.mem.dout", (4, 128, hidden), 0.1))
    tlens = _dev(np.asarray([128, 100, 64, 128], np.int32))
    peaks = {}
    for key, kw in (("attention_precision=half", dict(attention_precision="half")), ("precision=half", dict(precision="half"))):
        layer = _layer(hidden, heads, inter, eps, sd, **kw)

        def run():
            layer.zero_grad(set_to_none=True)
            ths = hs.clone().requires_grad_(True)
            with torch.autocast("cuda", dtype=torch.float16):
                out = layer(ths, tlens)
            out.float().backward(tdout)

        run()   # warm-up: the allocator's pools, autocast's weight casts
        torch.cuda.synchronize()
        layer.zero_grad(set_to_none=True)
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        run()
        torch.cuda.synchronize()
        peaks[key] = torch.cuda.max_memory_allocated() - before
        del layer
    print("peak memory above the resident set, forward + backward, 4 x 128 rows: %r" % (peaks,))
    assert peaks["precision=half"] < peaks["attention_precision=half"], peaks


def test_bert_layer_half_dropout_is_finite_and_deterministic_and_needs_autocast():
    from ance_amd import _lib
    from ance_amd import attention as T
    sd = U.layer_weights(768, 3072)
    layer = _layer(768, 12, 3072, 1e-5, sd, 0.1, precision="half").train()
    hs = _dev(U.det_normal(3, "half.hs.768", (2, 40, 768), 1.0))
    lens = _dev(np.array([40, 9], np.int32))

    def run():
        T.manual_seed(11)
        layer.zero_grad(set_to_none=True)
        ths = hs.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16):
            out = layer(ths, lens)
        out.sum().backward()
        return [out.detach().clone(), ths.grad.clone()] + [p.grad.clone() for p in layer.parameters()]

    a, b = run(), run()
    for x, y in zip(a, b):
        assert bool(torch.isfinite(x).all()) and _same_bits(x, y)
    assert T.dropout_state.offsets[0] == 3   # the attention and the two tails, one pair each
    with pytest.raises(_lib.AnceLibraryError, match="float16 or bfloat16"):
        layer(hs, lens)   # fp32 hidden states outside autocast: nothing is cast behind the caller's back
