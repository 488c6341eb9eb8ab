"""The first-row attention core (ance_amd.attention.attention_first_row -> csrc/attention_row0.hip) on the GPU against the fp64
statement of tests/model_util.py.

Bound per tensor (ctx, dq, dk, dv): fp32 within attention_train_util.bound = max(4 x the eager fp32 expression's own distance from
fp64, 16 ulp32 of the fp64 tensor's largest magnitude); 16 bits within attention_half_util.bound16 = max(4 x the eager autocast
expression's distance, 2 ulp of the dtype), on inputs rounded to the dtype first.  tests/test_model.py holds the statement against
autograd on the CPU, so a failure here is the kernel's.  Every measured distance is printed."""
import functools

import numpy as np
import pytest
import torch

import attention_half_util as HU
import attention_train_util as A
import model_util as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 0x5EED0123456789AB
IO = {None: torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def _dev(x, dtype=None, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    if dtype is not None:
        t = t.to(dtype)
    return t.requires_grad_(True) if grad else t


def _np(t):
    return t.detach().float().cpu().numpy()


def _run(q0, k, v, g, lens, nh, dt=None, layout="separate", **kw):
    """attention_first_row and its backward.  layout "fused": k and v are thirds of one [B, L, 3H] buffer and q0 is row 0 of the
    first third, all passed as strided views."""
    from ance_amd.attention import attention_first_row
    io = IO[dt]
    if layout == "fused":
        B, L, H = k.shape
        q = np.zeros_like(k)
        q[:, 0] = q0
        fused = _dev(np.concatenate([q, k, v], axis=2), io, True)
        tq, tk, tv = fused[:, 0, :H], fused[:, :, H:2 * H], fused[:, :, 2 * H:]
        assert not tk.is_contiguous() and not tq.is_contiguous()
    else:
        tq, tk, tv = (_dev(x, io, True) for x in (q0, k, v))
    ctx = attention_first_row(tq, tk, tv, _dev(np.asarray(lens, np.int32)), nh, kw.get("dropout_p", 0.0), kw.get("training", True),
                              "fp32" if dt is None else "half")
    assert ctx.dtype == io and tuple(ctx.shape) == tuple(q0.shape)
    ctx.backward(_dev(g, io))
    if layout == "fused":
        gr = fused.grad
        assert gr.dtype == io
        assert np.all(_np(gr[:, 1:, :H]) == 0)
        return dict(ctx=_np(ctx), dq=_np(gr[:, 0, :H]), dk=_np(gr[:, :, H:2 * H]), dv=_np(gr[:, :, 2 * H:]))
    assert tq.grad.dtype == tk.grad.dtype == tv.grad.dtype == io
    return dict(ctx=_np(ctx), dq=_np(tq.grad), dk=_np(tk.grad), dv=_np(tv.grad))


_reference = functools.lru_cache(maxsize=None)(M.reference)


def _ref(tag, lens, nh, L=None, q_scale=1.0, p=0.0, offset=0, dt=None):
    return _reference(tag, tuple(lens), nh, L, q_scale, p, SEED, offset, None if dt is None else HU.DTYPES[dt])


def _pads_are_zero(got, lens):
    for b, n in enumerate(lens):
        assert np.all(got["dk"][b, n:] == 0) and np.all(got["dv"][b, n:] == 0), ("pad rows of dk / dv", b, n)
        if n == 0:
            assert np.all(got["ctx"][b] == 0) and np.all(got["dq"][b] == 0), ("a sequence of length 0", b)


# ---------------------------------------------------------------------------------------------------------------- 1. lengths
@pytest.mark.parametrize("nh", [12, 16])
@pytest.mark.parametrize("batch", range(len(M.SWEEP_BATCHES)))
def test_length_sweep_fp32(batch, nh):
    lens = M.SWEEP_BATCHES[batch]
    (q0, k, v, g, ln), want, ref, _ = _ref("sweep%d.%d" % (batch, nh), lens, nh)
    got = _run(q0, k, v, g, ln, nh)
    M.check("sweep %r %d heads fp32" % (lens, nh), got, want, ref)
    _pads_are_zero(got, lens)


@pytest.mark.parametrize("dt,nh", [("fp16", 12), ("bf16", 16), ("fp16", 16), ("bf16", 12)])
@pytest.mark.parametrize("batch", range(len(M.SWEEP_BATCHES)))
def test_length_sweep_half(batch, dt, nh):
    lens = M.SWEEP_BATCHES[batch]
    (q0, k, v, g, ln), want, ref, _ = _ref("sweep%d.%d" % (batch, nh), lens, nh, dt=dt)
    got = _run(q0, k, v, g, ln, nh, dt)
    M.check("sweep %r %d heads %s" % (lens, nh, dt), got, want, ref, HU.DTYPES[dt])
    _pads_are_zero(got, lens)


# ---------------------------------------------------------------------------------------------------------------- 2. dropout
DROP_LENS, DROP_L = (1, 5, 64, 130, 0), 131


@pytest.mark.parametrize("dt", [None, "fp16", "bf16"])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_dropout_matches_the_restated_philox_mask(p, dt):
    """The mask restated on the CPU under the call's own (seed, offset): a wrong counter shows as an O(1) error.  A second call
    advances the offset; p = 0 and training=False draw nothing."""
    from ance_amd import attention as T
    T.manual_seed(SEED)
    dtype = None if dt is None else HU.DTYPES[dt]
    (q0, k, v, g, ln), want, ref, _ = _ref("dropout", DROP_LENS, 12, DROP_L, 1.0, p, 0, dt)
    r0 = _run(q0, k, v, g, ln, 12, dt, dropout_p=p)
    M.check("dropout p=%g offset 0 %s" % (p, dt), r0, want, ref, dtype)
    _pads_are_zero(r0, DROP_LENS)
    assert T.dropout_state.offsets.get(0, 0) == (1 if p > 0 else 0)
    if p > 0:
        (_, want1, ref1, _) = _ref("dropout", DROP_LENS, 12, DROP_L, 1.0, p, 1, dt)
        r1 = _run(q0, k, v, g, ln, 12, dt, dropout_p=p)
        M.check("dropout p=%g offset 1 %s" % (p, dt), r1, want1, ref1, dtype)
        assert T.dropout_state.offsets.get(0, 0) == 2
        (_, want_e, ref_e, _) = _ref("dropout", DROP_LENS, 12, DROP_L, 1.0, 0.0, 0, dt)
        M.check("dropout p=%g training=False %s" % (p, dt), _run(q0, k, v, g, ln, 12, dt, dropout_p=p, training=False), want_e, ref_e, dtype)
        assert T.dropout_state.offsets.get(0, 0) == 2


def test_dropout_device_stream_draws_the_host_masks():
    """The _dstream entry points: after to_device the same calls give the host mode's bits, and a backward behind advance() is
    refused."""
    from ance_amd import _lib, attention as T
    (q0, k, v, g, ln), _, _, _ = _ref("dropout", DROP_LENS, 12, DROP_L, 1.0, 0.5, 0, None)
    T.manual_seed(SEED)
    host = [_run(q0, k, v, g, ln, 12, dropout_p=0.5) for _ in range(2)]
    T.manual_seed(SEED)
    T.dropout_state.to_device(0)
    try:
        dev = [_run(q0, k, v, g, ln, 12, dropout_p=0.5)]
        T.dropout_state.advance(0)
        dev.append(_run(q0, k, v, g, ln, 12, dropout_p=0.5))
        for a, b in zip(host, dev):
            for n in M.NAMES:
                assert np.array_equal(a[n], b[n]), n
        from ance_amd.attention import attention_first_row
        tq, tk, tv = (_dev(x, None, True) for x in (q0, k, v))
        ctx = attention_first_row(tq, tk, tv, _dev(ln), 12, 0.5, True)
        T.dropout_state.advance(0)
        with pytest.raises(_lib.AnceLibraryError, match="has moved"):
            ctx.backward(_dev(g))
    finally:
        T.dropout_state.to_host(0)
        T.manual_seed(SEED)


# ---------------------------------------------------------------------------------------------------------------- 3. saturated, layouts
@pytest.mark.parametrize("dt", [None, "fp16", "bf16"])
@pytest.mark.parametrize("scale", [8.0, 30.0])
def test_saturated_scores(scale, dt):
    (q0, k, v, g, ln), want, ref, _ = _ref("saturated", (33, 97), 12, 97, scale, dt=dt)
    M.check("saturated x%g %s" % (scale, dt), _run(q0, k, v, g, ln, 12, dt), want, ref, None if dt is None else HU.DTYPES[dt])


@pytest.mark.parametrize("dt", [None, "fp16", "bf16"])
def test_strided_views_and_two_runs_give_the_same_bits(dt):
    """k, v as thirds of a fused [B, L, 3H] buffer and q0 as row 0 of its first third give the bits of the separate tensors; a second
    run gives the same bits again."""
    lens = (96, 31, 0, 7)
    (q0, k, v, g, ln), want, ref, _ = _ref("layouts", lens, 12, 96, dt=dt)
    a = _run(q0, k, v, g, ln, 12, dt)
    M.check("layouts separate %s" % dt, a, want, ref, None if dt is None else HU.DTYPES[dt])
    b = _run(q0, k, v, g, ln, 12, dt, layout="fused")
    c = _run(q0, k, v, g, ln, 12, dt)
    for n in M.NAMES:
        assert np.array_equal(a[n], b[n]), ("fused", n)
        assert np.array_equal(a[n], c[n]), ("second run", n)
    _pads_are_zero(b, lens)


# ---------------------------------------------------------------------------------------------------------------- 4. the full core's row 0
@pytest.mark.parametrize("dt", [None, "fp16"])
def test_mask_identity_with_the_full_core(dt):
    """Under the same (seed, offset) at p = 0.5 the call equals row 0 of attention_padded, and with dctx nonzero in row 0 only the full
    core's dk, dv and dq[:, 0] equal this kernel's, within the bound of the sweep -- a mask that differed in one element would show
    as an O(1) error.  The lengths cross the full core's 32-key blocks and 64-row tiles; the tiny ones are the sweep's (at length 1
    dS is exactly 0 here, while the full core, which takes D from the stored ctx, leaves its rounding noise times P = 1)."""
    from ance_amd import attention as T
    p, nh, lens, L = 0.5, 12, (70, 33, 128, 65), 128
    io = IO[dt]
    dtype = None if dt is None else HU.DTYPES[dt]
    (q0, k, v, g, ln), want, ref, _ = _ref("identity", lens, nh, L, 1.0, p, 0, dt)
    T.manual_seed(SEED)
    got = _run(q0, k, v, g, ln, nh, dt, dropout_p=p)
    M.check("identity first-row %s" % dt, got, want, ref, dtype)
    q = A.seeded_inputs("identity.q", lens, nh, L=L)[0]
    if dtype is not None:
        q = HU.round16(q, dtype)
    q[:, 0] = q0
    dctx = np.zeros_like(q)
    dctx[:, 0] = g
    T.manual_seed(SEED)
    tq, tk, tv = (_dev(x, io, True) for x in (q, k, v))
    full = T.attention_padded(tq, tk, tv, _dev(ln), nh, p, True, "fp32" if dt is None else "half")
    full.backward(_dev(dctx, io))
    core = dict(ctx=_np(full[:, 0]), dq=_np(tq.grad[:, 0]), dk=_np(tk.grad), dv=_np(tv.grad))
    assert np.all(_np(tq.grad[:, 1:]) == 0)
    for n in M.NAMES:
        d = float(np.abs(core[n].astype(np.float64) - got[n]).max())
        big = float(np.abs(want[n]).max())
        b = A.bound(ref[n], big) if dtype is None else HU.bound16(ref[n], big, dtype)
        print("identity %s %-4s |full core - first row| %.3e  bound %.3e" % (dt, n, d, b))
        assert d <= b, (n, d, b)


# ---------------------------------------------------------------------------------------------------------------- 5. arguments
def test_argument_checks():
    from ance_amd import _lib
    from ance_amd.attention import attention_first_row
    q0, k, v, lens = torch.zeros(2, 768, device=DEV), torch.zeros(2, 8, 768, device=DEV), torch.zeros(2, 8, 768, device=DEV), \
        torch.tensor([8, 3], device=DEV)
    for bad in (lambda: attention_first_row(q0[:1], k, v, lens, 12), lambda: attention_first_row(q0, k, v, lens, 16),
                lambda: attention_first_row(q0, k, v[:, :4], lens, 12), lambda: attention_first_row(q0.half(), k, v, lens, 12),
                lambda: attention_first_row(q0, k, v, lens, 12, precision="half"), lambda: attention_first_row(q0, k, v, lens[:1], 12),
                lambda: attention_first_row(q0, k, v, lens, 12, dropout_p=1.0), lambda: attention_first_row(q0.cpu(), k, v, lens, 12)):
        with pytest.raises(_lib.AnceLibraryError):
            bad()


def test_capturable():
    """Forward and backward inside a captured graph: the replay gives the eager bits."""
    from ance_amd.attention import attention_first_row
    (q0, k, v, g, ln), _, _, _ = _ref("layouts", (96, 31, 0, 7), 12, 96)
    eager = _run(q0, k, v, g, ln, 12)
    tq, tk, tv, tg, tl = _dev(q0, None, True), _dev(k, None, True), _dev(v, None, True), _dev(g), _dev(ln)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up off the default stream, as torch asks
        attention_first_row(tq, tk, tv, tl, 12).backward(tg)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    tq.grad = tk.grad = tv.grad = None
    with torch.cuda.graph(graph):
        ctx = attention_first_row(tq, tk, tv, tl, 12)
        ctx.backward(tg)
    ctx.zero_()
    graph.replay()
    torch.cuda.synchronize()
    got = dict(ctx=_np(ctx), dq=_np(tq.grad), dk=_np(tk.grad), dv=_np(tv.grad))
    for n in M.NAMES:
        assert np.array_equal(eager[n], got[n]), n
