"""The 16-bit attention core (ance_amd/attention.py precision="half" -> csrc/attention_train_half.hip) on the GPU against the fp64
restatement of tests/attention_train_util.py on the SAME 16-bit-valued inputs.

Bound, per 16-bit tensor (ctx, dq, dk, dv): max |got - fp64| <= bound16 = max(4 x D_ref, 2 ulp of the dtype at the fp64 tensor's
largest magnitude), D_ref the eager autocast expression's own distance from fp64 (attention_half_util.eager_half on the CPU); the fp32
log-sum-exp is held to A.bound against eager_half's lse distance.  tests/test_attention_half.py pins on the CPU that a model of the
kernels' contract meets these bounds on the seeded cases, so a failure here is the kernels'.  Every measured distance is printed."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import attention_half_util as HU
import attention_train_util as A

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BOTH = ["fp16", "bf16"]


def _dev(x, dtype=None, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    if dtype is not None:
        t = t.to(dtype)
    return t.requires_grad_(True) if grad else t


def _np(t):
    return t.detach().float().cpu().numpy()


def _run_padded(q, k, v, g, lens, nh, dtype, **kw):
    from ance_amd.attention import _padded
    tq, tk, tv = (_dev(x, dtype, True) for x in (q, k, v))
    ctx, lse = _padded(tq, tk, tv, _dev(np.asarray(lens, np.int32)), nh, kw.get("dropout_p", 0.0), kw.get("training", True), "half")
    assert ctx.dtype == dtype and lse.dtype == torch.float32 and not lse.requires_grad
    ctx.backward(_dev(g, dtype))
    assert tq.grad.dtype == tk.grad.dtype == tv.grad.dtype == dtype
    return dict(ctx=_np(ctx), lse=_np(lse), dq=_np(tq.grad), dk=_np(tk.grad), dv=_np(tv.grad))


def _run_packed(q, k, v, g, lens, nh, dtype, **kw):
    from ance_amd.attention import _packed
    lens = np.asarray(lens, np.int32)
    L = q.shape[1]
    (pq, off), pk, pv, pg = A.pack(q, lens), A.pack(k, lens)[0], A.pack(v, lens)[0], A.pack(g, lens)[0]
    tq, tk, tv = (_dev(x, dtype, True) for x in (pq, pk, pv))
    ctx, lse = _packed(tq, tk, tv, _dev(off), L, nh, kw.get("dropout_p", 0.0), kw.get("training", True), "half")
    ctx.backward(_dev(pg, dtype))
    out = {n: A.unpack(_np(t), lens, L) for n, t in (("ctx", ctx), ("dq", tq.grad), ("dk", tk.grad), ("dv", tv.grad))}
    out["lse"] = A.unpack(_np(lse).T.copy(), lens, L).transpose(2, 0, 1).reshape(nh, len(lens) * L)
    return out


_seeded = functools.lru_cache(maxsize=None)(HU.seeded_reference)
_sweep = functools.lru_cache(maxsize=None)(HU.sweep_reference)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------- 1. one-hot, exact
@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("n", [32, 64, 96, 512])
def test_one_hot_permutation_is_exact(n, dt):
    """P is exactly one-hot, so ctx[i] = v[pi(i)], dv[pi(i)] = dctx[i] and dq = dk = 0, bit for bit: a wrong k order in either forward
    product or in the dV product shows with the row indices in hand."""
    q, k, v, g, pi = HU.one_hot_case(n)
    got = _run_padded(q, k, v, g, [n], 12, HU.DTYPES[dt])
    for h in range(12):
        c = slice(64 * h, 64 * h + 64)
        want_ctx = v[0, pi[h], c]
        bad = np.argwhere((got["ctx"][0, :, c] != want_ctx).any(axis=1)).ravel()
        assert bad.size == 0, ("ctx: query rows, and the key rows they should have copied", h, bad[:8], pi[h][bad[:8]])
        want_dv = np.zeros((n, 64), np.float32)
        want_dv[pi[h]] = g[0, :, c]
        bad = np.argwhere((got["dv"][0, :, c] != want_dv).any(axis=1)).ravel()
        assert bad.size == 0, ("dv", h, bad[:8])
        assert np.all(got["lse"][h, :n] == 504.0), ("lse", h)
    assert np.all(got["dq"] == 0) and np.all(got["dk"] == 0)


# ---------------------------------------------------------------------------------------------------------------- 2. lengths
def test_length_sweep_12_heads_packed_fp16():
    (q, k, v, g, ln), want, ref = _sweep(A.SWEEP_LENS, 12, "fp16")
    HU.check("sweep 12 heads packed fp16", _run_packed(q, k, v, g, ln, 12, torch.float16), want, ref, torch.float16)


def test_length_sweep_16_heads_padded_bf16():
    (q, k, v, g, ln), want, ref = _sweep(A.SWEEP_LENS_16, 16, "bf16")
    HU.check("sweep 16 heads padded bf16", _run_padded(q, k, v, g, ln, 16, torch.bfloat16), want, ref, torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------- 3. golden
@functools.lru_cache(maxsize=None)
def _golden_reference(golden_dir, case, dt):
    dtype = HU.DTYPES[dt]
    with open(os.path.join(golden_dir, "attention_train.json")) as f:
        meta = json.load(f)
    g = np.load(os.path.join(golden_dir, "attention_train.npz"))
    m, nh = meta[case], meta["n_heads"]
    lens, L = np.asarray(m["lens"], np.int32), m["L"]
    x = [HU.round16(A.unpack(g["%s.%s" % (case, n)], lens, L), dtype) for n in ("q", "k", "v", "dctx")]
    want = A.attention_fp64(*x, lens, nh)
    return x, lens, nh, want, A.distances(HU.eager_half(*x, lens, nh, dtype), want)


@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("case", A.GOLDEN_CASES)
def test_golden_padded_and_packed(golden_dir, case, dt):
    """The reference's own q, k, v, dctx of both towers, rounded to the dtype."""
    x, lens, nh, want, ref = _golden_reference(golden_dir, case, dt)
    for form, run in (("padded", _run_padded), ("packed", _run_packed)):
        HU.check("golden %s %s %s" % (case, form, dt), run(*x, lens, nh, HU.DTYPES[dt]), want, ref, HU.DTYPES[dt])


# ---------------------------------------------------------------------------------------------------------------- 4. dropout
@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_matches_the_restated_philox_mask(p, dt):
    """The mask restated on the CPU under the call's own (seed, offset): a wrong counter shows as an O(1) error.  A second call
    advances the offset; training=False and p = 0 draw nothing and give the no-dropout bits."""
    from ance_amd import attention as T
    dtype, seed, L = HU.DTYPES[dt], HU.DROPOUT_SEED, 130
    T.manual_seed(seed)
    (q, k, v, g, ln), want, ref, _ = _seeded("dropout", A.DROPOUT_LENS, 12, L, 1.0, p, seed, 0, dt)
    r0 = _run_padded(q, k, v, g, ln, 12, dtype, dropout_p=p)
    HU.check("dropout p=%g offset 0 %s" % (p, dt), r0, want, ref, dtype)
    assert T.dropout_state.offsets.get(0, 0) == 1
    r1 = _run_padded(q, k, v, g, ln, 12, dtype, dropout_p=p)
    (_, want1, ref1, _) = _seeded("dropout", A.DROPOUT_LENS, 12, L, 1.0, p, seed, 1, dt)
    HU.check("dropout p=%g offset 1 %s" % (p, dt), r1, want1, ref1, dtype)
    assert T.dropout_state.offsets.get(0, 0) == 2
    for n in ("ctx", "dq", "dk", "dv"):
        assert not np.array_equal(r0[n], r1[n]), n
    assert np.array_equal(r0["lse"], r1["lse"])
    plain = _run_padded(q, k, v, g, ln, 12, dtype)
    before = dict(T.dropout_state.offsets)
    for kw in (dict(dropout_p=p, training=False), dict(dropout_p=0.0, training=True)):
        r = _run_padded(q, k, v, g, ln, 12, dtype, **kw)
        for n in A.NAMES:
            assert np.array_equal(_bits(plain[n]), _bits(r[n])), (kw, n)
    assert T.dropout_state.offsets == before


# ---------------------------------------------------------------------------------------------------------------- 5. saturation
@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("scale", [8.0, 30.0])
def test_saturated_softmax(scale, dt):
    (q, k, v, g, ln), want, ref, _ = _seeded("saturated.%g" % scale, (33, 97), 12, 97, scale, 0.0, 0, 0, dt)
    HU.check("saturated x%g %s" % (scale, dt), _run_padded(q, k, v, g, ln, 12, HU.DTYPES[dt]), want, ref, HU.DTYPES[dt])


# ---------------------------------------------------------------------------------------------------------------- 6. layouts
LAYOUT_LENS, LAYOUT_L = (96, 31, 0), 96


@pytest.mark.parametrize("dt", BOTH)
def test_layouts_fused_and_separate_agree_bitwise_and_pad_rows_are_zero(dt):
    """Views of a fused [B, L, 3H] and three tensors give the same bits, gradients included; pad rows of ctx, dq, dk, dv are +0.0 with
    NaN-filled pad rows of q, k, v and dctx, the length-0 sequence included."""
    from ance_amd.attention import _padded
    dtype = HU.DTYPES[dt]
    (q, k, v, g, ln), want, ref, _ = _seeded("layouts", LAYOUT_LENS, 12, LAYOUT_L, 1.0, 0.0, 0, 0, dt)
    rows = np.arange(LAYOUT_L)[None, :] < ln[:, None]
    qn, kn, vn, gn = (np.where(rows[:, :, None], x, np.float32("nan")) for x in (q, k, v, g))
    lens = _dev(ln)
    res = []
    for form in ("separate", "fused"):
        if form == "separate":
            tq, tk, tv = (_dev(x, dtype, True) for x in (qn, kn, vn))
            leaves = (tq, tk, tv)
        else:
            fused = _dev(np.concatenate([qn, kn, vn], axis=-1), dtype, True)
            tq, tk, tv = fused[..., :768], fused[..., 768:1536], fused[..., 1536:]
            assert not tq.is_contiguous()
            leaves = (fused,)
        ctx, lse = _padded(tq, tk, tv, lens, 12, 0.0, True, "half")
        ctx.backward(_dev(gn, dtype))
        if form == "separate":
            grads = [_np(t.grad) for t in leaves]
        else:
            assert fused.grad.dtype == dtype
            gf = _np(fused.grad)
            grads = [gf[..., :768], gf[..., 768:1536], gf[..., 1536:]]
        res.append(dict(ctx=_np(ctx), lse=_np(lse), dq=grads[0], dk=grads[1], dv=grads[2]))
    for n in A.NAMES:
        assert np.array_equal(_bits(res[0][n]), _bits(res[1][n])), n
    for n in ("ctx", "dq", "dk", "dv"):
        assert np.all(_bits(res[0][n][~rows]) == 0), n
    HU.check("layouts (96, 31, 0) %s" % dt, res[0], want, ref, dtype)


def test_packed_form_leaves_uncovered_rows_alone():
    """The C ABI in the packed form on caller-owned buffers: rows that no sequence covers, the guard rows and the stride's unused
    columns keep their sentinel in ctx, dq, dk and dv."""
    import ctypes
    from ance_amd import _lib
    L_ = _lib.lib()
    dtype, SENT = torch.float16, 0x7DAB   # a NaN with a recognisable payload
    (q, k, v, g, ln), want, ref, _ = _seeded("layouts", LAYOUT_LENS, 12, LAYOUT_L, 1.0, 0.0, 0, 0, "fp16")
    B, Lq, H, G, ld = len(ln), LAYOUT_L, 768, 5, 768 + 8
    all_rows = B * Lq
    rows = (np.arange(Lq)[None, :] < ln[:, None]).reshape(-1)

    def guarded(x=None):
        buf = torch.full((all_rows + 2 * G, ld), SENT, dtype=torch.int16, device=DEV).view(dtype)
        if x is not None:
            buf[G:G + all_rows, :H] = _dev(x.reshape(all_rows, H), dtype)
        return buf

    bq, bk, bv, bg = guarded(q), guarded(k), guarded(v), guarded(g)
    outs = dict(ctx=guarded(), dq=guarded(), dk=guarded(), dv=guarded())
    ws_bytes = L_.ance_attention16_workspace_bytes(all_rows, 12)
    ws = torch.zeros(ws_bytes // 4, dtype=torch.float32, device=DEV)
    first = _dev(np.array([0, Lq, 2 * Lq, all_rows + 7, -3], np.int32))
    lens = _dev(np.array([200, 31, 0, 50, 20], np.int32))   # 200 is clamped to max_seq_len; the last two start outside [0, n_rows)
    P = lambda t: t[G:].data_ptr()  # noqa: E731
    a = _lib.AnceAttn16Args(q=P(bq), k=P(bk), v=P(bv), ctx=P(outs["ctx"]), ld_q=ld, ld_k=ld, ld_v=ld, ld_ctx=ld,
                            d_seq_first=first.data_ptr(), d_seq_len=lens.data_ptr(), n_seq=5, max_seq_len=Lq, n_rows=all_rows,
                            n_heads=12, seq_rows=0, dtype=_lib.ANCE_DTYPE_F16, dropout_p=0.0, training=1, seed=0, offset=0,
                            d_workspace=ws.data_ptr(), workspace_bytes=ws_bytes)
    gr = _lib.AnceAttn16GradArgs(dctx=P(bg), dq=P(outs["dq"]), dk=P(outs["dk"]), dv=P(outs["dv"]), ld_dctx=ld, ld_dq=ld, ld_dk=ld, ld_dv=ld)
    st = _lib.current_stream_ptr()
    _lib.check(L_.ance_attention16_forward(ctypes.byref(a), st), "forward")
    _lib.check(L_.ance_attention16_backward(ctypes.byref(a), ctypes.byref(gr), st), "backward")
    torch.cuda.synchronize()
    got = {}
    for n, buf in outs.items():
        bits = buf.view(torch.int16).cpu().numpy()
        assert np.all(bits[:G] == SENT) and np.all(bits[G + all_rows:] == SENT), n + ": guard rows"
        assert np.all(bits[:, H:] == SENT), n + ": columns past 64 n_heads"
        assert np.all(bits[G:G + all_rows, :H][~rows] == SENT), n + ": rows that no sequence covers"
        x = np.zeros((all_rows, H), np.float32)
        x[rows] = _np(buf)[G:G + all_rows, :H][rows]
        got[n] = x.reshape(B, Lq, H)
    got["lse"] = np.where(rows[None, :], _np(ws)[:12 * all_rows].reshape(12, all_rows), 0)
    HU.check("C ABI packed, stride 776", got, want, ref, dtype)


def test_padded_form_zeroes_its_pad_rows_and_leaves_the_rest_alone():
    """The padded_rule twin of the test above, in bf16 (seq_rows = L): the pad rows of the 31-row sequence and the rows of the empty
    one are written as exact zeros by the call itself into sentinel-filled ctx, dq, dk and dv -- up to an n_rows that ends inside the
    buffer, 40 rows into the empty sequence: nothing at or behind it is touched.  Guard rows, the stride's unused columns and the
    NaN-filled workspace's guards keep their bits; a length above max_seq_len is clamped; descriptors that start outside [0, n_rows)
    touch nothing.  The guards are wide enough for a kernel without its clamps to stay inside the buffers."""
    import ctypes
    from ance_amd import _lib
    L_ = _lib.lib()
    dtype, SENT, NAN32 = torch.bfloat16, 0x7FCB, 0x7FC00ABC   # NaNs with a recognisable payload
    (q, k, v, g, ln), want, ref, _ = _seeded("layouts", LAYOUT_LENS, 12, LAYOUT_L, 1.0, 0.0, 0, 0, "bf16")
    B, Lq, H, G, ld = len(ln), LAYOUT_L, 768, 64, 768 + 8
    all_rows, n_rows = B * Lq, 2 * Lq + 40
    valid = (np.arange(Lq)[None, :] < ln[:, None]).reshape(-1)
    inside = np.arange(all_rows) < n_rows
    # a first row at n_rows + 7 with seq_rows = 96 rows behind it, and one at -3, stay inside the guards even without clamps
    assert n_rows + 7 + Lq <= all_rows + G and 3 <= G and 200 <= all_rows + G

    def guarded(x=None):
        buf = torch.full((all_rows + 2 * G, ld), SENT, dtype=torch.int16, device=DEV).view(dtype)
        if x is not None:
            buf[G:G + all_rows, :H] = _dev(x.reshape(all_rows, H), dtype)
        return buf

    ins = dict(q=guarded(q), k=guarded(k), v=guarded(v), dctx=guarded(np.where(valid.reshape(B, Lq)[:, :, None], g, np.float32("nan"))))
    before = {n: t.view(torch.int16).clone() for n, t in ins.items()}
    outs = dict(ctx=guarded(), dq=guarded(), dk=guarded(), dv=guarded())
    ws_bytes = L_.ance_attention16_workspace_bytes(n_rows, 12)
    ws = torch.full((ws_bytes // 4 + 2 * 64,), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
    first = _dev(np.array([0, Lq, 2 * Lq, n_rows + 7, -3], np.int32))
    lens = _dev(np.array([200, 31, 0, 50, 20], np.int32))   # 200 is clamped to max_seq_len; the last two start outside [0, n_rows)
    P = lambda t: t[G:].data_ptr()  # noqa: E731
    a = _lib.AnceAttn16Args(q=P(ins["q"]), k=P(ins["k"]), v=P(ins["v"]), ctx=P(outs["ctx"]), ld_q=ld, ld_k=ld, ld_v=ld, ld_ctx=ld,
                            d_seq_first=first.data_ptr(), d_seq_len=lens.data_ptr(), n_seq=5, max_seq_len=Lq, n_rows=n_rows,
                            n_heads=12, seq_rows=Lq, dtype=_lib.ANCE_DTYPE_BF16, dropout_p=0.0, training=1, seed=0, offset=0,
                            d_workspace=ws[64:].data_ptr(), workspace_bytes=ws_bytes)
    gr = _lib.AnceAttn16GradArgs(dctx=P(ins["dctx"]), dq=P(outs["dq"]), dk=P(outs["dk"]), dv=P(outs["dv"]), ld_dctx=ld, ld_dq=ld,
                                 ld_dk=ld, ld_dv=ld)
    st = _lib.current_stream_ptr()
    _lib.check(L_.ance_attention16_forward(ctypes.byref(a), st), "forward")
    _lib.check(L_.ance_attention16_backward(ctypes.byref(a), ctypes.byref(gr), st), "backward")
    torch.cuda.synchronize()
    got = {}
    for n, buf in outs.items():
        bits = buf.view(torch.int16).cpu().numpy()
        assert np.all(bits[:G] == SENT) and np.all(bits[G + all_rows:] == SENT), n + ": guard rows"
        assert np.all(bits[:, H:] == SENT), n + ": columns past 64 n_heads"
        body = bits[G:G + all_rows, :H]
        assert np.all(body[~valid & inside] == 0), n + ": pad rows below n_rows are written as +0.0"
        assert np.all(body[~inside] == SENT), n + ": nothing at or behind n_rows is touched"
        x = np.zeros((all_rows, H), np.float32)
        x[valid] = _np(buf)[G:G + all_rows, :H][valid]
        assert np.all(np.isfinite(x)), n
        got[n] = x.reshape(B, Lq, H)
    for n, t in ins.items():
        assert torch.equal(t.view(torch.int16), before[n]), n + " has changed"
    wbits = ws.view(torch.int32).cpu().numpy()
    assert np.all(wbits[:64] == NAN32) and np.all(wbits[64 + ws_bytes // 4:] == NAN32), "workspace guards"
    got["lse"] = np.zeros((12, all_rows), np.float32)
    got["lse"][:, :n_rows] = np.where(valid[None, :n_rows], _np(ws)[64:64 + 12 * n_rows].reshape(12, n_rows), 0)
    HU.check("C ABI padded bf16, stride 776", got, want, ref, dtype)


# ---------------------------------------------------------------------------------------------------------------- 7. determinism
@pytest.mark.parametrize("dt", BOTH)
def test_deterministic_capturable_and_never_synchronises(dt):
    from ance_amd import attention as T
    dtype = HU.DTYPES[dt]
    q, k, v, g, ln = HU.rounded_inputs("capture", (70, 33, 0, 128), 12, dtype, L=128)
    tin = [_dev(x, dtype) for x in (q, k, v, g)]
    lens = _dev(ln)
    mask = (torch.arange(128, device=DEV)[None, :] < lens[:, None]).long()

    def step(p):
        tq, tk, tv = (t.clone().requires_grad_(True) for t in tin[:3])
        ctx = T.attention_padded(tq, tk, tv, T.lens_from_mask(mask), 12, dropout_p=p, precision="half")
        ctx.backward(tin[3])
        return [ctx.detach(), tq.grad, tk.grad, tv.grad]

    for p in (0.0, 0.1):
        T.manual_seed(5)
        e1 = [t.clone() for t in step(p)]
        T.manual_seed(5)
        e2 = [t.clone() for t in step(p)]
        torch.cuda.synchronize()
        for x, y in zip(e1, e2):
            assert torch.equal(x.view(torch.int16), y.view(torch.int16))
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
            step(p)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        T.manual_seed(5)
        with torch.cuda.graph(graph):
            outs = step(p)
        for _ in range(2):
            for t in outs:
                t.zero_()
            graph.replay()
            torch.cuda.synchronize()
            for x, y in zip(e1, outs):
                assert torch.equal(x.view(torch.int16), y.view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------- 8. overflow
def test_overflow_reaches_the_scaler_fp16():
    """dctx times 2^20: the fp64 dS exceeds 2 x 65504 (asserted), so the fp16 dS is +-inf and dq or dk must hold a non-finite value
    for GradScaler's found_inf -- a saturating conversion would hand over a clamped, finite gradient.  At a scale where the fp64 dS,
    dq, dk, dv all stay below 2^14 everything is finite and within bound16.  Only inf values are produced; nothing faults."""
    dtype, lens = torch.float16, (2, 5)

    def fp64_ds(q, k, v, g, ln):
        rows = A._valid(ln, q.shape[1])
        Q, K, V = (A._heads(np.asarray(x, np.float64), 12) for x in (q, k, v))
        G = A._heads(np.where(rows[:, :, None], np.asarray(g, np.float64), 0.0), 12)
        S = Q @ K.transpose(0, 1, 3, 2) * 0.125 + ((1.0 - rows) * -10000.0)[:, None, None, :]
        P = np.exp(S - S.max(-1, keepdims=True))
        P /= P.sum(-1, keepdims=True)
        dP = G @ V.transpose(0, 1, 3, 2)
        return np.where(rows[:, None, :, None], P * (dP - (dP * P).sum(-1, keepdims=True)), 0.0)

    q, k, v, g0, ln = HU.rounded_inputs("overflow", lens, 12, dtype)
    # the scaled incoming gradient as a GradScaler hands it over: fp32 values times 2^20, clamped into fp16's finite range so that
    # the overflow under test is the kernel's own dS, not an inf that was already in its input
    g = HU.round16(np.clip(A.seeded_inputs("overflow", lens, 12)[3] * np.float32(2.0 ** 20), -65504.0, 65504.0), dtype)
    assert np.isfinite(g).all()
    assert np.abs(fp64_ds(q, k, v, g, ln)).max() > 2 * 65504.0
    got = _run_padded(q, k, v, g, ln, 12, dtype)
    assert not (np.isfinite(got["dq"]).all() and np.isfinite(got["dk"]).all())
    # the issue's own input, unclamped (its elements above 65504 are already inf in fp16): non-finite as well
    g_inf = HU.round16(A.seeded_inputs("overflow", lens, 12)[3] * np.float32(2.0 ** 20), dtype)
    with np.errstate(invalid="ignore"):
        assert not np.abs(fp64_ds(q, k, v, g_inf, ln)).max() <= 2 * 65504.0
    got = _run_padded(q, k, v, g_inf, ln, 12, dtype)
    assert not (np.isfinite(got["dq"]).all() and np.isfinite(got["dk"]).all())
    # a scale that keeps everything below 2^14
    scale = 2.0 ** 10
    (q, k, v, g, ln), want, ref, _ = HU.seeded_reference("overflow", lens, 12, 5, 1.0, 0.0, 0, 0, "fp16", g_scale=scale)
    assert max(np.abs(fp64_ds(q, k, v, g, ln)).max(), *(np.abs(want[n]).max() for n in ("dq", "dk", "dv"))) < 2.0 ** 14
    got = _run_padded(q, k, v, g, ln, 12, dtype)
    assert all(np.isfinite(got[n]).all() for n in A.NAMES)
    HU.check("scaled by 2^10 fp16", got, want, ref, dtype)


# ---------------------------------------------------------------------------------------------------------------- 9. the fp32 core
@pytest.mark.parametrize("dt", BOTH)
def test_against_the_fp32_core_on_the_device(dt):
    """The fp32 core on the same 16-bit-valued inputs: both are within their bounds of fp64, so within the sum of the two of each other."""
    from ance_amd.attention import _padded
    dtype = HU.DTYPES[dt]
    (q, k, v, g, ln), want, ref, _ = _seeded("vs32", (70, 33, 128), 12, 128, 1.0, 0.0, 0, 0, dt)
    got = _run_padded(q, k, v, g, ln, 12, dtype)
    HU.check("vs32 half %s" % dt, got, want, ref, dtype)
    tq, tk, tv = (_dev(x, None, True) for x in (q, k, v))
    ctx, lse = _padded(tq, tk, tv, _dev(ln), 12, 0.0, True)
    ctx.backward(_dev(g))
    got32 = dict(ctx=_np(ctx), lse=_np(lse), dq=_np(tq.grad), dk=_np(tk.grad), dv=_np(tv.grad))
    ref32 = A.distances(A.eager_fp32(q, k, v, g, ln, 12), want)
    b16 = HU.bounds(ref, want, dtype)
    for n in A.NAMES:
        b32 = A.bound(ref32[n], np.abs(want[n]).max())
        d32 = float(np.abs(got32[n].astype(np.float64) - want[n]).max())
        d = float(np.abs(got[n].astype(np.float64) - got32[n]).max())
        print("vs32 %s %-4s fp32 core vs fp64 %.3e (bound %.3e)  half vs fp32 core %.3e (bound %.3e)" % (dt, n, d32, b32, d, b16[n] + b32))
        assert d32 <= b32 and d <= b16[n] + b32, (n, d32, b32, d, b16[n])


# ---------------------------------------------------------------------------------------------------------------- 10. BertLayer
def _eager_layer(hs, rows, W, nh, eps):
    """transformers' eager BertLayer with torch ops (dropout 0), ctx zeroed at pad rows as ance_amd.layers.BertLayer leaves it."""
    F = torch.nn.functional
    B, L, H = hs.shape

    def heads(x):
        return x.view(B, L, nh, 64).permute(0, 2, 1, 3)

    def lin(x, name, bias=True):
        return F.linear(x, W[name + ".weight"], W[name + ".bias"] if bias else None)

    q, k, v = (lin(hs, "attention.self." + n) for n in ("query", "key", "value"))
    mask = ((1.0 - rows.float()) * -10000.0)[:, None, None, :]
    scores = torch.matmul(heads(q), heads(k).transpose(-1, -2)) / 8.0 + mask
    probs = torch.softmax(scores, dim=-1)
    ctx = torch.matmul(probs, heads(v)).permute(0, 2, 1, 3).contiguous().view(B, L, H)
    ctx = ctx * rows[:, :, None].to(ctx.dtype)
    ln = "attention.output.LayerNorm"
    h = F.layer_norm(lin(ctx, "attention.output.dense") + hs, (H,), W[ln + ".weight"], W[ln + ".bias"], eps)
    t = lin(h, "intermediate.dense")
    t = t * 0.5 * (1.0 + torch.erf(t / 1.4142135623730951))
    ln = "output.LayerNorm"
    return F.layer_norm(lin(t, "output.dense") + h, (H,), W[ln + ".weight"], W[ln + ".bias"], eps)


@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("lens,hidden,heads,inter", [((40, 9), 768, 12, 3072), ((17,), 1024, 16, 4096)])
def test_bert_layer_half_attention_under_autocast(lens, hidden, heads, inter, dt):
    """BertLayer(attention_precision="half") under torch.autocast: the attention receives and returns the autocast dtype; the output
    and the gradients of the input and of every parameter are within 4 x D of the fp32 BertLayer (outside autocast) on the same
    weights, D = |eager autocast layer - the fp32 BertLayer| per tensor.  The measured ratios are printed."""
    import layer_tail_util as U
    from ance_amd import attention as T
    from ance_amd.layers import BertLayer
    dtype, eps = HU.DTYPES[dt], 1e-5
    B, L = len(lens), max(lens)
    sd = U.layer_weights(hidden, inter)
    hs = U.det_normal(3, "half.hs.%d" % hidden, (B, L, hidden), 1.0)
    rows_np = A._valid(np.asarray(lens), L)
    dout = np.where(rows_np[:, :, None], U.det_normal(3, "half.dout.%d" % hidden, (B, L, hidden), 0.1), np.float32(0))
    rows, tlens, tdout = _dev(rows_np), _dev(np.asarray(lens, np.int32)), _dev(dout)

    def run_layer(precision, autocast):
        layer = BertLayer(hidden, heads, inter, eps, 0.0, 0.0, attention_precision=precision).to(DEV)
        layer.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        ths = _dev(hs, None, True)
        with torch.autocast("cuda", dtype=dtype, enabled=autocast):
            out = layer(ths, tlens)
        out.float().backward(tdout)
        res = {k: _np(p.grad) for k, p in layer.named_parameters()}
        res["out"], res["dhs"] = (np.where(rows_np[:, :, None], _np(t), 0.0) for t in (out, ths.grad))
        return res

    seen = []
    real = T._padded

    def spy(q, k, v, *a, **kw):
        r = real(q, k, v, *a, **kw)
        seen.append((q.dtype, k.dtype, v.dtype, r[0].dtype))
        return r

    T._padded = spy
    try:
        got = run_layer("half", True)
    finally:
        T._padded = real
    assert seen == [(dtype,) * 4], seen
    base = run_layer("fp32", False)
    W = {k: _dev(v, None, True) for k, v in sd.items()}
    ths = _dev(hs, None, True)
    with torch.autocast("cuda", dtype=dtype):
        out = _eager_layer(ths, rows, W, heads, eps)
    out.float().backward(tdout)
    eager = {k: _np(w.grad) for k, w in W.items()}
    eager["out"], eager["dhs"] = (np.where(rows_np[:, :, None], _np(t), 0.0) for t in (out, ths.grad))
    bad, worst = [], 0.0
    for n in sorted(base):
        D = float(np.abs(eager[n].astype(np.float64) - base[n]).max())
        d = float(np.abs(got[n].astype(np.float64) - base[n]).max())
        worst = max(worst, d / max(D, 1e-300))
        print("BertLayer half %s H %d %-36s |half - fp32| %.3e  D = |eager autocast - fp32| %.3e  ratio %5.2f" % (dt, hidden, n, d, D, d / max(D, 1e-300)))
        if not d <= 4.0 * D:
            bad.append((n, d, D))
    print("BertLayer half %s H %d largest ratio %.2f" % (dt, hidden, worst))
    assert not bad, bad


def test_bert_layer_half_dropout_is_finite_and_deterministic_and_needs_autocast():
    import layer_tail_util as U
    from ance_amd import _lib
    from ance_amd import attention as T
    from ance_amd.layers import BertLayer
    sd = U.layer_weights(768, 3072)
    layer = BertLayer(768, 12, 3072, 1e-5, 0.1, 0.1, attention_precision="half").to(DEV).train()
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    hs = _dev(U.det_normal(3, "half.hs.768", (2, 40, 768), 1.0))
    lens = _dev(np.array([40, 9], np.int32))

    def run():
        T.manual_seed(11)
        layer.zero_grad(set_to_none=True)
        ths = hs.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16):
            out = layer(ths, lens)
        out.float().sum().backward()
        return [out.detach().clone(), ths.grad.clone()] + [p.grad.clone() for p in layer.parameters()]

    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.isfinite(x).all() and torch.equal(x, y)
    with pytest.raises(_lib.AnceLibraryError, match="float16 or bfloat16"):
        layer(hs, lens)
