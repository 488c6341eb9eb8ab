"""The BertLayer's row-wise seams (ance_amd/layers.py -> csrc/layer_tail.hip) on the GPU against the fp64 restatements of
tests/layer_tail_util.py and the reference's own tensors (tests/golden/layer_tail*.npz).

Bound, per tensor:  max |got - fp64| <= max(4 x D_ref, 16 ulp32 of the fp64 tensor's largest magnitude), D_ref the eager fp32
expression's own distance from fp64: the fixture's recorded ones for the golden cases, the torch CPU evaluation of the same inputs and
the same mask for the seeded ones.  Every measured distance is printed: delta, reference, ratio, bound."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import attention_train_util as A
import layer_tail_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN32 = 0x7FC00ABC   # the sentinel: a NaN with a recognisable payload
SEED = 0x5EED0123456789AB


def _dev(x, grad=False):
    if x is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t.requires_grad_(True) if grad else t


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check(tag, got, want, ref_err, names):
    bad = []
    for n in names:
        if want[n] is None:
            continue
        d = float(np.abs(np.asarray(got[n], np.float64) - want[n]).max())
        b = U.bound(ref_err[n], np.abs(want[n]).max())
        print("%-44s %-6s max|delta| %.3e  reference %.3e  ratio %6.2f  bound %.3e" % (tag, n, d, ref_err[n], d / max(ref_err[n], 1e-300), b))
        if not d <= b:
            bad.append((n, d, b))
    assert not bad, (tag, bad)


def _run_tail(x, b, r, g, be, eps, dy, p=0.0, training=True):
    from ance_amd.layers import dropout_add_layer_norm
    tx, tb, tr, tg, tbe = (_dev(t, True) for t in (x, b, r, g, be))
    y = dropout_add_layer_norm(tx, tb, tr, tg, tbe, eps, p, training)
    y.backward(_dev(dy))
    return dict(y=_np(y), dx=_np(tx.grad), dres=_np(tr.grad), dgamma=_np(tg.grad), dbeta=_np(tbe.grad), dbias=_np(tb.grad) if tb is not None else None)


def _run_gelu(x, b, dy):
    from ance_amd.layers import bias_gelu
    tx, tb = _dev(x, True), _dev(b, True)
    y = bias_gelu(tx, tb)
    y.backward(_dev(dy))
    return dict(y=_np(y), dx=_np(tx.grad), dbias=_np(tb.grad))


@functools.lru_cache(maxsize=None)
def _tail_reference(tag, n_rows, H, p, eps, offset=0):
    """Seeded inputs, the fp64 restatement and the eager fp32 expression's distances under the mask of (SEED, offset): once, on the CPU."""
    inp = U.tail_inputs(tag, n_rows, H)
    keep = U.tail_keep_mask(p, SEED, offset, n_rows, H) if p > 0 else None
    want = U.tail_fp64(*inp[:5], eps, inp[5], keep, p)
    ref = U.distances(U.tail_eager_fp32(*inp[:5], eps, inp[5], keep, p), want, U.TAIL_NAMES)
    return inp, keep, want, ref


@functools.lru_cache(maxsize=None)
def _gelu_reference(tag, n_rows, N):
    inp = U.gelu_inputs(tag, n_rows, N)
    want = U.gelu_fp64(*inp)
    return inp, want, U.distances(U.gelu_eager_fp32(*inp), want, U.GELU_NAMES)


def _row_counts():
    from ance_amd import _lib
    R = _lib.LAYER_TAIL_ROWS_PER_WORKGROUP   # the kernels' rows per workgroup, as the library states it
    assert _lib.lib().ance_layer_tail_rows_per_workgroup() == R
    # 3 R + 5: three full partial rows and a remainder; 130 R + 5: more than eight partial rows per slice of the reducer's tree
    return sorted({1, 2, 3, 4, 5, 63, 64, 65, R - 1, R, R + 1, 3 * R + 5, 130 * R + 5})


# ------------------------------------------------------------------------------------------------------------------------ golden
@pytest.mark.parametrize("case", U.GOLDEN_CASES)
def test_golden_seams(golden_dir, case):
    """Both towers' own tensors at the three seams: every output and gradient against fp64 within the bound set by the reference's
    own fp32-to-fp64 distance and by the eager expression's distance on the committed inputs, and next to the reference's fp32 results."""
    m, seams = U.load_golden(golden_dir, case)
    for seam in U.SEAMS:
        t, rec, names = seams[seam], m["seams"][seam], U.seam_names(seam)
        want = U.golden_fp64(seam, t, m["eps"])
        if seam in U.TAILS:
            got = _run_tail(t["x"], t["bias"], t["res"], t["gamma"], t["beta"], m["eps"], t["dy"], 0.1, False)   # eval mode: no dropout
            names = names + ("dres",)
            ref_err, same = dict(rec["ref_err"], dres=rec["ref_err"]["dx"]), dict(rec["same_inputs"], dres=rec["same_inputs"]["dx"])
            theirs = dict(t, dres=t["dx"])   # eval mode: the reference's dres is its dx
        else:
            got, ref_err, same, theirs = _run_gelu(t["x"], t["bias"], t["dy"]), rec["ref_err"], rec["same_inputs"], t
        _check("golden %s %s" % (case, seam), got, want, ref_err, names)
        _check("golden %s %s, same inputs" % (case, seam), got, want, same, names)
        for n in names:   # the reference's fp32 tensors: both are within the bound of fp64, so within twice it of each other
            d = float(np.abs(got[n].astype(np.float64) - theirs[n]).max())
            b = 2 * U.bound(ref_err[n], np.abs(want[n]).max())
            print("golden %s %s %-6s vs the reference's fp32 %.3e  bound %.3e" % (case, seam, n, d, b))
            assert d <= b, (seam, n, d, b)


# ------------------------------------------------------------------------------------------------------------------------ row sweep
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("H", [768, 1024])
def test_tail_row_sweep(H, p):
    from ance_amd import attention as T
    for n_rows in _row_counts():
        inp, keep, want, ref = _tail_reference("sweep.%d" % H, n_rows, H, p, 1e-5)
        T.manual_seed(SEED)   # offset 0
        got = _run_tail(*inp[:5], 1e-5, inp[5], p)
        _check("tail H %d p %.1f rows %d" % (H, p, n_rows), got, want, ref, U.TAIL_NAMES)


@pytest.mark.parametrize("N", [3072, 4096])
def test_gelu_row_sweep(N):
    for n_rows in _row_counts():
        inp, want, ref = _gelu_reference("sweep.%d" % N, n_rows, N)
        _check("gelu N %d rows %d" % (N, n_rows), _run_gelu(*inp), want, ref, U.GELU_NAMES)


# ------------------------------------------------------------------------------------------------------------------------ hard rows
@pytest.mark.parametrize("eps", [1e-5, 1e-12])
def test_hard_rows_for_the_layer_norm(eps):
    H, n = 768, 21
    x, b, r, g, be, dy = U.tail_inputs("hard", n, H)

    def both(tag, *inp):
        want = U.tail_fp64(*inp[:5], eps, inp[5])
        ref = U.distances(U.tail_eager_fp32(*inp[:5], eps, inp[5]), want, U.TAIL_NAMES)
        got = _run_tail(*inp[:5], eps, inp[5])
        _check("%s eps %g" % (tag, eps), got, want, ref, U.TAIL_NAMES)
        return got

    # mean 100, spread 0.01: E[z^2] - mean^2 in fp32 has no correct digit here
    both("mean 100 spread 0.01", (100.0 + 0.01 * x).astype(np.float32), b * np.float32(0.01), np.zeros_like(r), g, be, dy)
    # rows that are exactly constant, bias = res = 0: xhat is exactly 0 and y is beta, bit for bit.  The constants have short
    # mantissas, so every partial sum of 768 of them is exact in fp32 in any order and the mean is the constant itself.
    const = (np.arange(n, dtype=np.float32)[:, None] - 7.0) * np.float32(0.375) + np.zeros((n, H), np.float32)
    for bias in (np.zeros(H, np.float32), None):
        got = both("constant rows", const, bias, np.zeros_like(r), g, be, dy)
        assert np.array_equal(_bits(got["y"]), _bits(np.broadcast_to(be, (n, H)))), "y must equal beta bit for bit"
        assert np.all(got["dgamma"] == 0)
    # a quarter of gamma exactly 0, beta nonzero: xhat cannot be taken from (y - beta) / gamma
    g0 = g.copy()
    g0[::4] = 0.0
    assert np.all(be != 0)
    got = both("gamma with zeros", x, b, r, g0, be, dy)
    assert np.all(np.isfinite(got["dgamma"])) and np.abs(got["dgamma"][::4]).max() > 0
    # no bias: no dbias
    got = both("bias None", x, None, r, g, be, dy)
    assert got["dbias"] is None


# ------------------------------------------------------------------------------------------------------------------------ GELU range
def test_gelu_range():
    """u at +-0, +-1e-4, +-1, +-5, +-10, +-40: one column block of 256 per value; row 0 holds the values themselves, rows 1 .. 3 the
    values times (1 + k / 1024), so the eager expression's distance is a maximum over 1024 points near each value, not one point's
    luck.  The bound is taken per block, with the block's own magnitude."""
    vals = [0.0, -0.0, 1e-4, -1e-4, 1.0, -1.0, 5.0, -5.0, 10.0, -10.0, 40.0, -40.0]
    N = 256 * len(vals)
    u = np.repeat(np.asarray(vals, np.float32), 256)[None, :] * np.ones((4, 1), np.float32)
    u[1:] *= (1.0 + np.arange(3 * N, dtype=np.float32).reshape(3, N) % 768 / 1024.0)
    x, b, dy = u.astype(np.float32), np.zeros(N, np.float32), np.ones((4, N), np.float32)
    want, eager, got = U.gelu_fp64(x, b, dy), U.gelu_eager_fp32(x, b, dy), _run_gelu(x, b, dy)
    for n in U.GELU_NAMES:
        assert np.all(np.isfinite(got[n])), n
    for i, v in enumerate(vals):
        c = slice(256 * i, 256 * i + 256)
        blk = lambda d: {n: d[n][:, c] for n in ("y", "dx")}   # noqa: E731
        _check("gelu u = %g" % v, blk(got), blk(want), U.distances(blk(eager), blk(want), ("y", "dx")), ("y", "dx"))
    big, small = slice(256 * 10, 256 * 11), slice(256 * 11, 256 * 12)
    assert np.array_equal(got["y"][:, big], x[:, big]) and np.all(got["dx"][:, big] == 1.0)       # the tail is exactly u, the gradient 1
    assert np.all(got["y"][:, small] == 0.0) and np.all(got["dx"][:, small] == 0.0)               # exactly 0 and 0
    assert np.all(got["y"][0, :512] == 0.0) and np.all(got["dx"][0, :512] == 0.5)
    _check("gelu range", got, want, U.distances(eager, want, ("dbias",)), ("dbias",))


# ------------------------------------------------------------------------------------------------------------------------ strides
def test_strided_views_give_the_contiguous_bits():
    from ance_amd import attention as T
    from ance_amd.layers import bias_gelu, dropout_add_layer_norm
    H, n = 768, 37
    (x, b, r, g, be, dy), _, _, _ = _tail_reference("strides", n, H, 0.5, 1e-5)
    res = []
    for form in ("contiguous", "thirds", "vectors inside a flat buffer"):
        if form == "thirds":
            wide = _dev(np.concatenate([x, r, np.full_like(x, np.nan)], axis=1), True)
            tx, tr = wide[:, :H], wide[:, H:2 * H]
            assert tx.stride(0) == 3 * H and not tr.is_contiguous()
        else:
            tx, tr = _dev(x, True), _dev(r, True)
        if form == "vectors inside a flat buffer":   # as a flattened parameter store hands them out: 4-byte aligned only
            flat = _dev(np.concatenate([np.zeros(1, np.float32), b, g, be]), True)
            tb, tg, tbe = flat[1:H + 1], flat[H + 1:2 * H + 1], flat[2 * H + 1:]
            assert tb.data_ptr() % 16 == 4
        else:
            tb, tg, tbe = _dev(b, True), _dev(g, True), _dev(be, True)
        T.manual_seed(SEED)
        y = dropout_add_layer_norm(tx, tb, tr, tg, tbe, 1e-5, 0.5, True)
        grads = torch.autograd.grad(y, [tx, tr, tb, tg, tbe], _dev(dy))
        res.append([_np(y)] + [_np(t) for t in grads])
    for other in res[1:]:
        for a, c in zip(res[0], other):
            assert np.array_equal(_bits(a), _bits(c))
    (gx, gb, gdy), _, _ = _gelu_reference("strides", n, 3072)
    wide = _dev(np.concatenate([gx, np.full_like(gx, np.nan)], axis=1), True)
    out = []
    for tx in (_dev(gx, True), wide[:, :3072]):
        tb = _dev(gb, True)
        y = bias_gelu(tx, tb)
        out.append([_np(y)] + [_np(t) for t in torch.autograd.grad(y, [tx, tb], _dev(gdy))])
    for a, c in zip(*out):
        assert np.array_equal(_bits(a), _bits(c))
    # fp32 rows whose stride is 4 mod 8 (a 16-byte piece is 4 floats; 8 is the 16-bit rows' rule), one row past a 16-row workgroup
    n = 17
    x, b, r, g, be, dy = U.tail_inputs("stride 772", n, H)
    res = []
    for tx in (_dev(x, True), _dev(np.concatenate([x, np.full((n, 4), np.nan, np.float32)], axis=1), True)[:, :H]):
        tr, tb, tg, tbe = _dev(r, True), _dev(b, True), _dev(g, True), _dev(be, True)
        T.manual_seed(SEED)
        y = dropout_add_layer_norm(tx, tb, tr, tg, tbe, 1e-5, 0.5, True)
        res.append([_np(y)] + [_np(t) for t in torch.autograd.grad(y, [tx, tr, tb, tg, tbe], _dev(dy))])
    assert tx.stride(0) == 772 and tx.data_ptr() % 16 == 0
    for a, c in zip(*res):
        assert np.array_equal(_bits(a), _bits(c))
    gx, gb, gdy = U.gelu_inputs("stride 3076", n, 3072)
    out = []
    for tx in (_dev(gx, True), _dev(np.concatenate([gx, np.full((n, 4), np.nan, np.float32)], axis=1), True)[:, :3072]):
        tb = _dev(gb, True)
        y = bias_gelu(tx, tb)
        out.append([_np(y)] + [_np(t) for t in torch.autograd.grad(y, [tx, tb], _dev(gdy))])
    assert tx.stride(0) == 3076 and tx.data_ptr() % 16 == 0
    for a, c in zip(*out):
        assert np.array_equal(_bits(a), _bits(c))


class _Guarded:
    """A [rows, width] fp32 window at row stride ld inside a buffer of sentinels: guard rows in front and behind, guard columns
    between the rows."""

    def __init__(self, rows, width, ld, x=None, guard=3):
        self.rows, self.width, self.guard = rows, width, guard
        self.buf = torch.full((rows + 2 * guard, ld), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
        if x is not None:
            self.buf[guard:guard + rows, :width] = _dev(x.reshape(rows, width))

    @property
    def ptr(self):
        return self.buf[self.guard:].data_ptr()

    def window(self):
        return _np(self.buf)[self.guard:self.guard + self.rows, :self.width]

    def guards_intact(self):
        bits = _np(self.buf.view(torch.int32))
        g = self.guard
        return bool(np.all(bits[:g] == NAN32) and np.all(bits[g + self.rows:] == NAN32) and np.all(bits[:, self.width:] == NAN32))

    def untouched(self):
        return bool(np.all(_np(self.buf.view(torch.int32)) == NAN32))


def _tail_c_call(n, H, p, offset):
    """The tail's C ABI on guarded buffers (x and res at stride 3 H, as thirds of one buffer): args, grads, the buffers."""
    from ance_amd import _lib
    L_ = _lib.lib()
    (x, b, r, g, be, dy), keep, want, ref = _tail_reference("strides", n, H, p, 1e-5, offset)
    wide = _Guarded(n, 3 * H, 3 * H, np.concatenate([x, r, np.full_like(x, np.nan)], axis=1), guard=0)
    bufs = dict(y=_Guarded(n, H, H + 8), dx=_Guarded(n, H, H + 12), dres=_Guarded(n, H, H + 4), dy=_Guarded(n, H, H + 8, dy),
                dgamma=_Guarded(1, H, H), dbeta=_Guarded(1, H, H), dbias=_Guarded(1, H, H))
    vec = {k: _dev(v) for k, v in (("bias", b), ("gamma", g), ("beta", be))}
    ws_bytes = L_.ance_layer_tail_workspace_bytes(n, H)
    ws = _Guarded(1, ws_bytes // 4, ws_bytes // 4)
    a = _lib.AnceLayerTailArgs(x=wide.ptr, res=wide.ptr + 4 * H, bias=vec["bias"].data_ptr(), gamma=vec["gamma"].data_ptr(),
                               beta=vec["beta"].data_ptr(), y=bufs["y"].ptr, ld_x=3 * H, ld_res=3 * H, ld_y=H + 8, H=H, n_rows=n, eps=1e-5,
                               dropout_p=p, training=1, seed=SEED, offset=offset, d_workspace=ws.ptr, workspace_bytes=ws_bytes)
    gr = _lib.AnceLayerTailGradArgs(dy=bufs["dy"].ptr, dx=bufs["dx"].ptr, dres=bufs["dres"].ptr, dgamma=bufs["dgamma"].ptr,
                                    dbeta=bufs["dbeta"].ptr, dbias=bufs["dbias"].ptr, ld_dy=H + 8, ld_dx=H + 12, ld_dres=H + 4)
    return a, gr, bufs, ws, (wide, vec), want, ref


def test_c_abi_writes_only_its_window():
    """Through ctypes, outputs inside NaN-payload guard regions at row strides above the width: no guard word changes -- not in the
    gaps between the rows, not behind the last row, not around the column sums or the workspace."""
    from ance_amd import _lib
    L_ = _lib.lib()
    st = _lib.current_stream_ptr()
    n, H = 37, 768
    a, gr, bufs, ws, keepalive, want, ref = _tail_c_call(n, H, 0.5, 3)
    _lib.check(L_.ance_layer_tail_forward(ctypes.byref(a), st), "forward")
    _lib.check(L_.ance_layer_tail_backward(ctypes.byref(a), ctypes.byref(gr), st), "backward")
    torch.cuda.synchronize()
    for name, buf in list(bufs.items()) + [("workspace", ws)]:
        assert buf.guards_intact(), name
    got = {k: bufs[k].window() for k in ("y", "dx", "dres")}
    got.update({k: bufs[k].window()[0] for k in ("dgamma", "dbeta", "dbias")})
    _check("C ABI tail, strides 3H / H + 8", got, want, ref, U.TAIL_NAMES)
    # every output is optional in the backward
    for k in ("dx", "dres", "dgamma", "dbeta", "dbias"):
        a2, gr2, bufs2, ws2, keepalive2, _, _ = _tail_c_call(n, H, 0.5, 3)
        setattr(gr2, k, None)
        _lib.check(L_.ance_layer_tail_forward(ctypes.byref(a2), st), "forward")
        _lib.check(L_.ance_layer_tail_backward(ctypes.byref(a2), ctypes.byref(gr2), st), "backward")
        torch.cuda.synchronize()
        assert bufs2[k].untouched(), k
        for o in ("dx", "dres", "dgamma", "dbeta", "dbias"):
            if o != k:
                assert np.array_equal(_bits(bufs2[o].window()), _bits(bufs[o].window())), (k, o)

    N = 3072
    (x, b, dy), want, ref = _gelu_reference("strides", n, N)
    bx, bdy, by, bdx, bdb = _Guarded(n, N, N + 4, x), _Guarded(n, N, N + 8, dy), _Guarded(n, N, N + 8), _Guarded(n, N, N + 4), _Guarded(1, N, N)
    tb = _dev(b)
    ws_bytes = L_.ance_bias_gelu_workspace_bytes(n, N)
    ws = _Guarded(1, ws_bytes // 4, ws_bytes // 4)
    ga = _lib.AnceBiasGeluArgs(x=bx.ptr, bias=tb.data_ptr(), y=by.ptr, ld_x=N + 4, ld_y=N + 8, N=N, n_rows=n, d_workspace=ws.ptr, workspace_bytes=ws_bytes)
    gg = _lib.AnceBiasGeluGradArgs(dy=bdy.ptr, dx=bdx.ptr, dbias=bdb.ptr, ld_dy=N + 8, ld_dx=N + 4)
    _lib.check(L_.ance_bias_gelu_forward(ctypes.byref(ga), st), "forward")
    _lib.check(L_.ance_bias_gelu_backward(ctypes.byref(ga), ctypes.byref(gg), st), "backward")
    torch.cuda.synchronize()
    for name, buf in (("x", bx), ("dy", bdy), ("y", by), ("dx", bdx), ("dbias", bdb), ("workspace", ws)):
        assert buf.guards_intact(), name
    _check("C ABI gelu, strides N + 4 / N + 8", dict(y=by.window(), dx=bdx.window(), dbias=bdb.window()[0]), want, ref, U.GELU_NAMES)


# ------------------------------------------------------------------------------------------------------------------------ refusals
def test_c_abi_refusals_leave_the_outputs_untouched():
    """Every invalid argument of include/ance_amd.h on real buffers: ANCE_E_INVALID, and no output or workspace word changes."""
    from ance_amd import _lib
    L_ = _lib.lib()
    st = _lib.current_stream_ptr()
    n, H = 37, 768
    a, gr, bufs, ws, keepalive, _, _ = _tail_c_call(n, H, 0.5, 0)
    need = L_.ance_layer_tail_workspace_bytes(n, H)
    both = [dict(H=512), dict(H=3072), dict(n_rows=0), dict(n_rows=-1), dict(x=None), dict(res=None), dict(gamma=None), dict(x=a.x + 4),
            dict(res=a.res + 8), dict(bias=a.bias + 4), dict(gamma=a.gamma + 4), dict(ld_x=H - 4), dict(ld_x=3 * H + 2), dict(ld_res=0),
            dict(dropout_p=1.0), dict(dropout_p=-0.25), dict(dropout_p=float("nan")), dict(eps=0.0), dict(eps=-1e-5),
            dict(d_workspace=None), dict(d_workspace=a.d_workspace + 4), dict(workspace_bytes=0)]
    fwd_only = [dict(y=None), dict(beta=None), dict(y=a.y + 4), dict(beta=a.beta + 8), dict(ld_y=H - 4), dict(ld_y=H + 2),
                dict(workspace_bytes=2 * 256 - 1)]
    bwd_only = [dict(workspace_bytes=need - 1)]
    bad_grads = [dict(dy=None), dict(dy=gr.dy + 4), dict(dx=gr.dx + 4), dict(dres=gr.dres + 8), dict(dgamma=gr.dgamma + 4),
                 dict(dbeta=gr.dbeta + 4), dict(dbias=gr.dbias + 4), dict(ld_dy=H - 4), dict(ld_dx=H + 2), dict(ld_dres=0)]

    def mutated(struct, kw):
        m = type(struct).from_buffer_copy(struct)
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    for kw in both + fwd_only:
        assert L_.ance_layer_tail_forward(ctypes.byref(mutated(a, kw)), st) == -1, kw
        assert b"ance_layer_tail_forward" in L_.ance_last_error()
    for kw in both + bwd_only:
        assert L_.ance_layer_tail_backward(ctypes.byref(mutated(a, kw)), ctypes.byref(gr), st) == -1, kw
    for kw in bad_grads:
        assert L_.ance_layer_tail_backward(ctypes.byref(a), ctypes.byref(mutated(gr, kw)), st) == -1, kw
    assert L_.ance_layer_tail_backward(ctypes.byref(a), None, st) == -1 and L_.ance_layer_tail_forward(None, st) == -1

    N = 3072
    (x, b, dy), _, _ = _gelu_reference("strides", n, N)
    tx, tb, tdy = _dev(x), _dev(b), _dev(dy)
    gb = dict(y=_Guarded(n, N, N), dx=_Guarded(n, N, N), dbias=_Guarded(1, N, N))
    gneed = L_.ance_bias_gelu_workspace_bytes(n, N)
    gws = _Guarded(1, gneed // 4, gneed // 4)
    ga = _lib.AnceBiasGeluArgs(x=tx.data_ptr(), bias=tb.data_ptr(), y=gb["y"].ptr, ld_x=N, ld_y=N, N=N, n_rows=n, d_workspace=gws.ptr, workspace_bytes=gneed)
    gg = _lib.AnceBiasGeluGradArgs(dy=tdy.data_ptr(), dx=gb["dx"].ptr, dbias=gb["dbias"].ptr, ld_dy=N, ld_dx=N)
    gboth = [dict(N=768), dict(N=4000), dict(n_rows=0), dict(x=None), dict(bias=None), dict(x=ga.x + 4), dict(bias=ga.bias + 8), dict(ld_x=N - 4),
             dict(ld_x=N + 2)]
    for kw in gboth + [dict(y=None), dict(y=ga.y + 4), dict(ld_y=N - 4)]:
        assert L_.ance_bias_gelu_forward(ctypes.byref(mutated(ga, kw)), st) == -1, kw
    for kw in gboth + [dict(d_workspace=None), dict(d_workspace=ga.d_workspace + 4), dict(workspace_bytes=gneed - 1)]:
        assert L_.ance_bias_gelu_backward(ctypes.byref(mutated(ga, kw)), ctypes.byref(gg), st) == -1, kw
    for kw in (dict(dy=None), dict(dy=gg.dy + 4), dict(dx=gg.dx + 4), dict(dbias=gg.dbias + 4), dict(ld_dy=N - 4), dict(ld_dx=N + 2)):
        assert L_.ance_bias_gelu_backward(ctypes.byref(ga), ctypes.byref(mutated(gg, kw)), st) == -1, kw
    assert L_.ance_bias_gelu_backward(ctypes.byref(ga), None, st) == -1
    torch.cuda.synchronize()
    for name, buf in list(bufs.items()) + [("workspace", ws), ("gelu workspace", gws)] + list(gb.items()):
        if name != "dy":
            assert buf.untouched(), name


# ------------------------------------------------------------------------------------------------------------------------ dropout
def test_dropout_mask_stream_and_seed():
    from ance_amd import attention as T
    H, n, p = 1024, 45, 0.5
    inp, keep, want, ref = _tail_reference("dropout", n, H, p, 1e-5, 0)
    T.manual_seed(SEED)
    before = dict(T.dropout_state.offsets)
    r0 = _run_tail(*inp[:5], 1e-5, inp[5], p)                                   # offset 0
    assert T.dropout_state.offsets[0] == before.get(0, 0) + 1                   # exactly one per dropout call
    assert np.array_equal(r0["dx"] != 0, keep), "the mask implied by dx == 0 is the restated one, element for element"
    assert np.all(r0["dres"] != 0)
    r1 = _run_tail(*inp[:5], 1e-5, inp[5], p)                                   # offset 1
    assert T.dropout_state.offsets[0] == before.get(0, 0) + 2
    _, keep1, want1, ref1 = _tail_reference("dropout", n, H, p, 1e-5, 1)
    assert np.array_equal(r1["dx"] != 0, keep1) and not np.array_equal(keep, keep1)
    _check("dropout p 0.5 offset 1", r1, want1, ref1, U.TAIL_NAMES)
    T.manual_seed(SEED)
    r2 = _run_tail(*inp[:5], 1e-5, inp[5], p)
    for k in U.TAIL_NAMES:
        assert np.array_equal(_bits(r0[k]), _bits(r2[k])), k
    plain = _run_tail(*inp[:5], 1e-5, inp[5])
    at = dict(T.dropout_state.offsets)
    for kw in (dict(p=p, training=False), dict(p=0.0, training=True)):
        r = _run_tail(*inp[:5], 1e-5, inp[5], **kw)
        for k in U.TAIL_NAMES:
            assert np.array_equal(_bits(plain[k]), _bits(r[k])), (kw, k)
    assert T.dropout_state.offsets == at                                        # no draw, no counter advance
    # one stream with the attention: its dropout call takes the next pair
    q = torch.zeros(1, 4, 768, device=DEV)
    T.attention_padded(q, q, q, torch.tensor([4], device=DEV, dtype=torch.int32), 12, dropout_p=0.1)
    assert T.dropout_state.offsets[0] == at[0] + 1


# ------------------------------------------------------------------------------------------------------------------------ determinism
def test_deterministic_capturable_and_never_synchronises():
    from ance_amd import attention as T
    from ance_amd.layers import bias_gelu, dropout_add_layer_norm
    H, N, n = 768, 3072, 70
    (x, b, r, g, be, dy), _, _, _ = _tail_reference("capture", n, H, 0.1, 1e-5)
    (gx, gb, gdy), _, _ = _gelu_reference("capture", n, N)
    tin = [_dev(t) for t in (x, b, r, g, be, dy, gx, gb, gdy)]

    def step(p):
        tx, tb, tr, tg, tbe = (t.clone().requires_grad_(True) for t in tin[:5])
        y = dropout_add_layer_norm(tx, tb, tr, tg, tbe, 1e-5, p, True)
        y.backward(tin[5])
        ux, ub = (t.clone().requires_grad_(True) for t in tin[6:8])
        z = bias_gelu(ux, ub)
        z.backward(tin[8])
        return [y.detach(), tx.grad, tb.grad, tr.grad, tg.grad, tbe.grad, z.detach(), ux.grad, ub.grad]

    for p in (0.0, 0.1):
        T.manual_seed(5)
        e1 = [t.clone() for t in step(p)]
        T.manual_seed(5)
        e2 = [t.clone() for t in step(p)]
        torch.cuda.synchronize()
        for a, c in zip(e1, e2):
            assert torch.equal(a.view(torch.int32), c.view(torch.int32))
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
                assert torch.equal(a.view(torch.int32), c.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------ autocast
def test_autocast_casts_the_inputs_to_fp32():
    from ance_amd.layers import bias_gelu, dropout_add_layer_norm
    (x, b, r, g, be, dy), _, _, _ = _tail_reference("autocast", 9, 768, 0.0, 1e-5)
    hx, hb, hr, hg, hbe = (_dev(t).half() for t in (x, b, r, g, be))
    with torch.autocast("cuda", dtype=torch.float16):
        y = dropout_add_layer_norm(hx, hb, hr, hg, hbe, 1e-5)
    assert y.dtype == torch.float32
    want = dropout_add_layer_norm(hx.float(), hb.float(), hr.float(), hg.float(), hbe.float(), 1e-5)
    assert torch.equal(y.view(torch.int32), want.view(torch.int32))
    (gx, gb, _), _, _ = _gelu_reference("autocast", 9, 3072)
    ux, ub = _dev(gx).half(), _dev(gb).half()
    with torch.autocast("cuda", dtype=torch.float16):
        z = bias_gelu(ux, ub)
    assert z.dtype == torch.float32 and torch.equal(z.view(torch.int32), bias_gelu(ux.float(), ub.float()).view(torch.int32))
    with pytest.raises(Exception, match="float32"):
        dropout_add_layer_norm(hx, hb, hr, hg, hbe, 1e-5)   # outside autocast nothing is cast behind the caller's back
    with pytest.raises(Exception, match="float32"):
        bias_gelu(ux, ub)


# ------------------------------------------------------------------------------------------------------------------------ BertLayer
LAYER_LENS, LAYER_L = (4, 7, 9), 9


@functools.lru_cache(maxsize=None)
def _layer_reference(hidden, heads, inter, eps, p, offset):
    """hidden_states, dout, the weights, the fp64 composition and the eager fp32 composition's distances, with the three masks of
    offsets n, n + 1, n + 2 in call order (attention, first tail, second tail)."""
    B, L = len(LAYER_LENS), LAYER_L
    lens = np.asarray(LAYER_LENS, np.int32)
    sd = U.layer_weights(hidden, inter)
    hs, dout = U.det_normal(3, "layer.hs.%d" % hidden, (B, L, hidden), 1.0), U.det_normal(3, "layer.dout.%d" % hidden, (B, L, hidden), 0.1)
    keeps = None
    if p > 0:
        keeps = (A.keep_masks(p, SEED, offset, lens, heads, L), U.tail_keep_mask(p, SEED, offset + 1, B * L, hidden),
                 U.tail_keep_mask(p, SEED, offset + 2, B * L, hidden))
    want = U.layer_fp64(hs, lens, sd, heads, eps, dout, keeps, p, p)
    eager = U.layer_torch(hs, lens, sd, heads, eps, dout, keeps, p, p)
    rows = A._valid(lens, L)
    for d in (want, eager):   # only valid rows of the output and of the input gradient are compared
        for n in ("out", "dhs"):
            d[n] = np.where(rows[:, :, None], d[n], 0.0)
    names = U.LAYER_PARAMS + ("out", "dhs")
    return hs, dout, sd, lens, rows, want, U.distances(eager, want, names), names


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("hidden,heads,inter,eps", [(768, 12, 3072, 1e-5), (1024, 16, 4096, 1e-12)])
def test_bert_layer_end_to_end(hidden, heads, inter, eps, p):
    """The output, the input gradient (valid rows) and every parameter gradient against the fp64 composition, dropout off (eval mode,
    no draw) and at 0.1 / 0.1 with the masks of offsets n, n + 1, n + 2.  attention.self.key.bias has no gradient at all (a softmax
    does not see a constant added to a row of scores): both sides hold rounding noise there, and it is the comparison nearest to
    its bound (measured 0.6 of it)."""
    from ance_amd import attention as T
    from ance_amd.layers import BertLayer
    offset = 4 if p else 0
    hs, dout, sd, lens, rows, want, ref, names = _layer_reference(hidden, heads, inter, eps, p, offset)
    layer = BertLayer(hidden, heads, inter, eps, 0.1, 0.1).to(DEV)
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)   # the reference layer's names
    T.manual_seed(SEED)
    if p:
        layer.train()
        for _ in range(offset):   # the three calls take offsets n, n + 1, n + 2
            T.dropout_state.next_pair(torch.device(DEV))
    else:
        layer.eval()
    ths = _dev(hs, True)
    out = layer(ths, _dev(lens))
    out.backward(_dev(np.where(rows[:, :, None], dout, np.float32(0))))   # the incoming gradient is zero at pad rows
    assert T.dropout_state.offsets.get(0, 0) == (offset + 3 if p else 0)
    got = {k: _np(v.grad) for k, v in layer.named_parameters()}
    got["out"], got["dhs"] = (np.where(rows[:, :, None], _np(t), 0.0) for t in (out, ths.grad))
    _check("BertLayer H %d p %.1f" % (hidden, p), got, want, ref, names)
