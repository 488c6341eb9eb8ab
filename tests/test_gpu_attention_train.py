"""The trainers' attention core (ance_amd/attention.py -> csrc/attention_train.hip) on the GPU against the fp64 restatement of
tests/attention_train_util.py and the reference's own tensors (tests/golden/attention_train.*).

Bound, per tensor (ctx, lse, dq, dk, dv):  max |got - fp64| <= max(4 x D_ref, 16 ulp32 of the fp64 tensor's largest magnitude), D_ref
the eager fp32 expression's own distance from fp64: the golden's recorded one for the golden cases, the torch CPU evaluation of the same
inputs and the same mask for the seeded ones.  Every measured distance is printed."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import attention_train_util as A

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN32 = 0x7FC00ABC   # the sentinel: a NaN with a recognisable payload


def _dev(x, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t.requires_grad_(True) if grad else t


def _np(t):
    return t.detach().cpu().numpy()


def _check(tag, got, want, ref_err, names=A.NAMES):
    bad = []
    for n in names:
        d = float(np.abs(np.asarray(got[n], np.float64) - want[n]).max())
        b = A.bound(ref_err[n], np.abs(want[n]).max())
        print("%-30s %-4s max|delta| %.3e  reference %.3e  ratio %5.2f  bound %.3e" % (tag, n, d, ref_err[n], d / max(ref_err[n], 1e-300), b))
        if not d <= b:
            bad.append((n, d, b))
    assert not bad, (tag, bad)


def _run_padded(q, k, v, g, lens, nh, **kw):
    """attention_padded forward + backward; dict of numpy results (lse [nh, B * L])."""
    from ance_amd.attention import _padded
    tq, tk, tv = (_dev(x, True) for x in (q, k, v))
    ctx, lse = _padded(tq, tk, tv, _dev(np.asarray(lens, np.int32)), nh, kw.get("dropout_p", 0.0), kw.get("training", True))
    ctx.backward(_dev(g))
    return dict(ctx=_np(ctx), lse=_np(lse), dq=_np(tq.grad), dk=_np(tk.grad), dv=_np(tv.grad))


def _run_packed(q, k, v, g, lens, nh, max_seq_len=None, **kw):
    """The same call through attention_packed on the valid rows; results unpacked to the padded form for comparison."""
    from ance_amd.attention import _packed
    lens = np.asarray(lens, np.int32)
    L = q.shape[1]
    (pq, off), pk, pv, pg = A.pack(q, lens), A.pack(k, lens)[0], A.pack(v, lens)[0], A.pack(g, lens)[0]
    tq, tk, tv = (_dev(x, True) for x in (pq, pk, pv))
    ctx, lse = _packed(tq, tk, tv, _dev(off), max_seq_len or L, nh, kw.get("dropout_p", 0.0), kw.get("training", True))
    ctx.backward(_dev(pg))
    out = {n: A.unpack(_np(t), lens, L) for n, t in (("ctx", ctx), ("dq", tq.grad), ("dk", tk.grad), ("dv", tv.grad))}
    out["lse"] = A.unpack(_np(lse).T.copy(), lens, L).transpose(2, 0, 1).reshape(nh, len(lens) * L)
    return out


@functools.lru_cache(maxsize=None)
def _seeded_reference(tag, lens, nh, L, q_scale, p, seed, offset):
    """Inputs, the fp64 restatement and the eager fp32 expression's distances, computed once per case on the CPU (the padded form,
    with the additive -10000 mask)."""
    q, k, v, g, ln = A.seeded_inputs(tag, lens, nh, L=L, q_scale=q_scale)
    Lp = q.shape[1]
    keep = A.keep_masks(p, seed, offset, ln, nh, Lp) if p > 0 else None
    want = A.attention_fp64(q, k, v, g, ln, nh, keep, p)
    ref = A.distances(A.eager_fp32(q, k, v, g, ln, nh, keep, p), want)
    return (q, k, v, g, ln), want, ref


@functools.lru_cache(maxsize=None)
def _sweep_reference(lens, nh):
    """The length sweep: every sequence restated on its own (L = its length), results laid into the padded form."""
    q, k, v, g, ln = A.seeded_inputs("sweep.%d" % nh, lens, nh)
    L = q.shape[1]
    want = {n: np.zeros((len(lens), L, 64 * nh)) for n in ("ctx", "dq", "dk", "dv")}
    want["lse"] = np.zeros((nh, len(lens) * L))
    ref = {n: 0.0 for n in A.NAMES}
    for b, n in enumerate(lens):
        one = [x[b:b + 1, :n] for x in (q, k, v, g)]
        w = A.attention_fp64(*one, [n], nh)
        for name, d in A.distances(A.eager_fp32(*one, [n], nh), w).items():
            ref[name] = max(ref[name], d)
        for name in ("ctx", "dq", "dk", "dv"):
            want[name][b, :n] = w[name][0]
        want["lse"][:, b * L:b * L + n] = w["lse"]
    return (q, k, v, g, ln), want, ref


# ------------------------------------------------------------------------------------------------------------------------ golden
@pytest.mark.parametrize("case", A.GOLDEN_CASES)
def test_golden_padded_and_packed(golden_dir, case):
    """Both towers' own q, k, v, dctx: the call's results against fp64 within the bound set by the reference's own fp32-to-fp64
    distance, and next to the reference's fp32 results themselves."""
    with open(os.path.join(golden_dir, "attention_train.json")) as f:
        meta = json.load(f)
    g = np.load(os.path.join(golden_dir, "attention_train.npz"))
    m, nh = meta[case], meta["n_heads"]
    lens, L = np.asarray(m["lens"], np.int32), m["L"]
    x = {n: A.unpack(g["%s.%s" % (case, n)], lens, L) for n in ("q", "k", "v", "dctx", "ctx", "dq", "dk", "dv")}
    want = A.attention_fp64(x["q"], x["k"], x["v"], x["dctx"], lens, nh)
    for form, run in (("padded", _run_padded), ("packed", _run_packed)):
        got = run(x["q"], x["k"], x["v"], x["dctx"], lens, nh)
        _check("golden %s %s" % (case, form), got, want, m["ref_err"])
        # ref_err is the distance between the reference's whole fp32 and fp64 runs, which fed the attention different q, k, v, dctx:
        # for the gradients it is 40 - 170 x what the eager expression itself loses on the committed inputs.  That distance is in
        # the fixture too, and holds the same results to the bound as the seeded cases have it.
        _check("golden %s %s, same inputs" % (case, form), got, want, dict(m["ref_fp32_vs_fp64_on_same_inputs"], lse=m["ref_err"]["lse"]))
        for n in ("ctx", "dq", "dk", "dv"):   # the reference's fp32 tensors: both are within the bound of fp64, so within twice it of each other
            d = float(np.abs(got[n].astype(np.float64) - x[n]).max())
            assert d <= 2 * A.bound(m["ref_err"][n], np.abs(want[n]).max()), (n, d)


# ------------------------------------------------------------------------------------------------------------------------ lengths
def test_length_sweep_12_heads_packed():
    (q, k, v, g, ln), want, ref = _sweep_reference(A.SWEEP_LENS, 12)
    _check("sweep 12 heads packed", _run_packed(q, k, v, g, ln, 12), want, ref)


def test_length_sweep_16_heads_padded():
    (q, k, v, g, ln), want, ref = _sweep_reference(A.SWEEP_LENS_16, 16)
    _check("sweep 16 heads padded", _run_padded(q, k, v, g, ln, 16), want, ref)


# ------------------------------------------------------------------------------------------------------------------------ layouts
LAYOUT_LENS, LAYOUT_L = (96, 31, 0), 96


def test_layouts_fused_and_separate_agree_bitwise_and_pad_rows_are_zero():
    from ance_amd.attention import _padded
    (q, k, v, g, ln), want, ref = _seeded_reference("layouts", LAYOUT_LENS, 12, LAYOUT_L, 1.0, 0.0, 0, 0)
    rows = np.arange(LAYOUT_L)[None, :] < ln[:, None]
    g_nan = np.where(rows[:, :, None], g, np.float32("nan"))   # whatever dctx holds at pad rows is ignored
    lens = _dev(ln)
    res = []
    for form in ("separate", "fused"):
        if form == "separate":
            tq, tk, tv = (_dev(x, True) for x in (q, k, v))
            leaves = (tq, tk, tv)
        else:
            fused = _dev(np.concatenate([q, k, v], axis=-1), True)
            tq, tk, tv = fused[..., :768], fused[..., 768:1536], fused[..., 1536:]
            assert not tq.is_contiguous()
            leaves = (fused,)
        ctx, lse = _padded(tq, tk, tv, lens, 12, 0.0, True)
        ctx.backward(_dev(g_nan))
        if form == "separate":
            grads = [_np(t.grad) for t in leaves]
        else:
            gf = _np(fused.grad)
            grads = [gf[..., :768], gf[..., 768:1536], gf[..., 1536:]]
        res.append(dict(ctx=_np(ctx), lse=_np(lse), dq=grads[0], dk=grads[1], dv=grads[2]))
    for n in A.NAMES:
        assert np.array_equal(res[0][n].view(np.int32), res[1][n].view(np.int32)), n
    for n in ("ctx", "dq", "dk", "dv"):
        assert np.all(res[0][n][~rows].view(np.int32) == 0), n    # exactly +0.0, sequence of length 0 included
    _check("layouts (96, 31, 0)", res[0], want, ref)


@pytest.mark.parametrize("mode", ["packed_rule", "padded_rule"])
def test_c_abi_writes_only_its_rows_and_leaves_the_guards(mode):
    """The C ABI on caller-owned buffers with sentinel guard rows in front of and behind every tensor.
    packed_rule (seq_rows = 0): valid rows are written; pad rows, the guards and the stride's unused columns keep their bytes; lengths
    are clamped to max_seq_len and to an n_rows that ends inside the buffers.
    padded_rule (seq_rows = L): the pad rows -- of the 31-row sequence and all of the empty one -- are written as zeros by the call
    itself (no pre-zeroing), everything else as above.  Descriptors that start outside [0, n_rows) touch nothing either way."""
    from ance_amd import _lib
    L_ = _lib.lib()
    (q, k, v, g, ln), want, ref = _seeded_reference("layouts", LAYOUT_LENS, 12, LAYOUT_L, 1.0, 0.0, 0, 0)
    B, Lq, H, G, ld = len(ln), LAYOUT_L, 768, 5, 768 + 8
    all_rows = B * Lq
    padded = mode == "padded_rule"
    # packed_rule: the call's n_rows ends with sequence 1's last valid row: nothing at or behind it may be touched
    n_rows = all_rows if padded else Lq + int(ln[1])
    rows = (np.arange(Lq)[None, :] < ln[:, None]).reshape(-1)

    def guarded(x=None):
        buf = torch.full((all_rows + 2 * G, ld), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
        if x is not None:
            buf[G:G + all_rows, :H] = _dev(x.reshape(all_rows, H))
        return buf

    bq, bk, bv, bg = guarded(q), guarded(k), guarded(v), guarded(np.where(rows.reshape(B, Lq)[:, :, None], g, np.float32("nan")))
    bctx, bdq, bdk, bdv = guarded(), guarded(), guarded(), guarded()
    ws_bytes = L_.ance_attention_workspace_bytes(n_rows, 12)
    ws = torch.full((ws_bytes // 4 + 2 * 64,), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
    # lengths above max_seq_len (sequence 0: 200 -> 96) and, under packed_rule, past n_rows (sequence 1: 60 -> 31) are clamped; a first
    # row at or past n_rows (a fourth descriptor; under packed_rule sequence 2 as well) or below 0 (a fifth) skips the sequence
    first = _dev(np.array([0, Lq, 2 * Lq, n_rows + 7, -3], np.int32))
    lens = _dev(np.array([200, 31 if padded else 60, 0 if padded else 40, 50, 20], np.int32))
    P = lambda t: t[G:].data_ptr()  # noqa: E731
    a = _lib.AnceAttnTrainArgs(q=P(bq), k=P(bk), v=P(bv), ctx=P(bctx), ld_q=ld, ld_k=ld, ld_v=ld, ld_ctx=ld,
                               d_seq_first=first.data_ptr(), d_seq_len=lens.data_ptr(), n_seq=5, max_seq_len=Lq, n_rows=n_rows, n_heads=12, seq_rows=Lq if padded else 0,
                               dropout_p=0.0, training=1, seed=0, offset=0, d_workspace=ws[64:].data_ptr(), workspace_bytes=ws_bytes)
    gr = _lib.AnceAttnGradArgs(dctx=P(bg), dq=P(bdq), dk=P(bdk), dv=P(bdv), ld_dctx=ld, ld_dq=ld, ld_dk=ld, ld_dv=ld)
    st = _lib.current_stream_ptr()
    _lib.check(L_.ance_attention_forward(ctypes.byref(a), st), "forward")
    _lib.check(L_.ance_attention_backward(ctypes.byref(a), ctypes.byref(gr), st), "backward")
    torch.cuda.synchronize()
    got = {}
    for n, buf in (("ctx", bctx), ("dq", bdq), ("dk", bdk), ("dv", bdv)):
        bits = _np(buf.view(torch.int32))
        assert np.all(bits[:G] == NAN32) and np.all(bits[G + all_rows:] == NAN32), n + ": guard rows"
        assert np.all(bits[:, H:] == NAN32), n + ": columns past 64 n_heads"
        if padded:
            assert np.all(bits[G:G + all_rows, :H][~rows] == 0), n + ": pad rows are written as +0.0"
        else:
            assert np.all(bits[G:G + all_rows, :H][~rows] == NAN32), n + ": pad rows and rows >= n_rows are not written"
        x = np.zeros((all_rows, H), np.float32)
        x[rows] = _np(buf)[G:G + all_rows, :H][rows]
        got[n] = x.reshape(B, Lq, H)
    wbits = _np(ws.view(torch.int32))
    assert np.all(wbits[:64] == NAN32) and np.all(wbits[64 + ws_bytes // 4:] == NAN32), "workspace guards"
    for buf, x in ((bq, q), (bk, k), (bv, v)):
        assert np.array_equal(_np(buf)[G:G + all_rows, :H].view(np.int32), x.reshape(all_rows, H).view(np.int32))
    got["lse"] = np.zeros((12, all_rows), np.float32)
    got["lse"][:, :n_rows] = np.where(rows[None, :n_rows], _np(ws)[64:64 + 12 * n_rows].reshape(12, n_rows), 0)
    _check("C ABI %s, stride 776" % mode, got, want, ref)


# ------------------------------------------------------------------------------------------------------------------------ saturation
@pytest.mark.parametrize("scale", [8.0, 30.0])
def test_saturated_softmax(scale):
    """q scaled by 8 and by 30 against the fp64 restatement WITH the additive -10000 mask on the padded form: skipping the pad keys
    is the reference's mask."""
    (q, k, v, g, ln), want, ref = _seeded_reference("saturated.%g" % scale, (130, 64, 5, 1), 12, 130, scale, 0.0, 0, 0)
    _check("saturated x%g padded" % scale, _run_padded(q, k, v, g, ln, 12), want, ref)


# ------------------------------------------------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_matches_the_restated_philox_mask(p):
    """ctx and the gradients under dropout against fp64 with the CPU-restated mask of the call's own (seed, offset): the forward's
    and the backward's masks at once.  Then: another offset changes the results, manual_seed reproduces the bits, training=False
    and p = 0 give the no-dropout bits."""
    from ance_amd import attention as T
    seed, L = 0x5EED0123456789AB, 130
    T.manual_seed(seed)
    (q, k, v, g, ln), want, ref = _seeded_reference("dropout", A.DROPOUT_LENS, 12, L, 1.0, p, seed, 0)
    r0 = _run_padded(q, k, v, g, ln, 12, dropout_p=p)                      # offset 0
    _check("dropout p=%g offset 0" % p, r0, want, ref)
    r1 = _run_padded(q, k, v, g, ln, 12, dropout_p=p)                      # offset 1
    (_, want1, ref1) = _seeded_reference("dropout", A.DROPOUT_LENS, 12, L, 1.0, p, seed, 1)
    _check("dropout p=%g offset 1" % p, r1, want1, ref1)
    for n in ("ctx", "dq", "dk", "dv"):
        assert not np.array_equal(r0[n], r1[n]), n
    assert np.array_equal(r0["lse"], r1["lse"])                            # the log-sum-exp is of the undropped scores
    T.manual_seed(seed)
    r2 = _run_padded(q, k, v, g, ln, 12, dropout_p=p)
    for n in A.NAMES:
        assert np.array_equal(r0[n].view(np.int32), r2[n].view(np.int32)), n
    plain = _run_padded(q, k, v, g, ln, 12)
    before = dict(T.dropout_state.offsets)
    for kw in (dict(dropout_p=p, training=False), dict(dropout_p=0.0, training=True)):
        r = _run_padded(q, k, v, g, ln, 12, **kw)
        for n in A.NAMES:
            assert np.array_equal(plain[n].view(np.int32), r[n].view(np.int32)), (kw, n)
    assert T.dropout_state.offsets == before                              # no RNG work, no counter advance


# ------------------------------------------------------------------------------------------------------------------------ determinism
def test_deterministic_capturable_and_never_synchronises():
    from ance_amd import attention as T
    (q, k, v, g, ln), _, _ = _seeded_reference("capture", (70, 33, 0, 128), 12, 128, 1.0, 0.0, 0, 0)
    tin = [_dev(x) for x in (q, k, v, g)]
    lens = _dev(ln)
    mask = (torch.arange(128, device=DEV)[None, :] < lens[:, None]).long()

    def step(p):
        tq, tk, tv = (t.clone().requires_grad_(True) for t in tin[:3])
        ctx = T.attention_padded(tq, tk, tv, T.lens_from_mask(mask), 12, dropout_p=p)
        ctx.backward(tin[3])
        return [ctx.detach(), tq.grad, tk.grad, tv.grad]

    for p in (0.0, 0.1):
        T.manual_seed(5)
        e1 = [t.clone() for t in step(p)]
        T.manual_seed(5)
        e2 = [t.clone() for t in step(p)]
        torch.cuda.synchronize()
        for x, y in zip(e1, e2):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
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
            for x, y in zip(e1, outs):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------ audit path
def test_ctx_agrees_with_the_audit_kernel():
    """The inference encoder's fp32 attention (ance_debug_attention kind 2, one thread per query) on the same packed rows: the same
    bound on both against fp64, and the same bound between the two -- not bit for bit, the order differs."""
    from ance_amd import _lib
    from ance_amd.attention import attention_packed
    lens = (65, 7, 128, 1)
    (q, k, v, g, ln), want, ref = _seeded_reference("audit", lens, 12, 128, 1.0, 0.0, 0, 0)
    (pq, off), pk, pv = A.pack(q, ln), A.pack(k, ln)[0], A.pack(v, ln)[0]
    qkv = _dev(np.concatenate([pq, pk, pv], axis=1))
    T_ = qkv.shape[0]
    ctx = attention_packed(qkv[:, :768], qkv[:, 768:1536], qkv[:, 1536:], _dev(off), 128, 12)
    audit = torch.zeros(T_, 768, device=DEV)
    dd = torch.empty(len(off) + 4, dtype=torch.int32, device=DEV)
    h = np.ascontiguousarray(off, dtype=np.int32)
    a = _lib.AnceAttnDebugArgs(kind=2, n_heads=12, n_seq=len(lens), max_seq_len=128, cls_only=0, q_compact=0, h_desc=h.ctypes.data,
                               d_desc=dd.data_ptr(), d_desc_bytes=dd.numel() * 4, qk=qkv.data_ptr(), ld_qk=qkv.stride(0), qk_rows=T_,
                               vt=None, ld_vt=0, ctx=audit.data_ptr(), ld_ctx=768, ctx_rows=T_)
    _lib.check(_lib.lib().ance_debug_attention(ctypes.byref(a), _lib.current_stream_ptr()), "ance_debug_attention")
    torch.cuda.synchronize()
    w = A.pack(want["ctx"], ln)[0]
    b = A.bound(ref["ctx"], np.abs(w).max())
    d1, d2 = (float(np.abs(_np(t).astype(np.float64) - w).max()) for t in (ctx, audit))
    d12 = float((ctx - audit).abs().max())
    print("ctx vs fp64 %.3e  audit kernel vs fp64 %.3e  ctx vs audit %.3e  bound %.3e" % (d1, d2, d12, b))
    assert d1 <= b and d2 <= b and d12 <= b


# ------------------------------------------------------------------------------------------------------------------------ autocast
def test_autocast_casts_the_inputs_to_fp32():
    from ance_amd.attention import attention_padded
    (q, k, v, g, ln), _, _ = _seeded_reference("autocast", (40, 9), 12, 40, 1.0, 0.0, 0, 0)
    hq, hk, hv = (_dev(x).half() for x in (q, k, v))
    lens = _dev(ln)
    with torch.autocast("cuda", dtype=torch.float16):
        ctx = attention_padded(hq, hk, hv, lens, 12)
    assert ctx.dtype == torch.float32
    want = attention_padded(hq.float(), hk.float(), hv.float(), lens, 12)
    assert torch.equal(ctx.view(torch.int32), want.view(torch.int32))
    with pytest.raises(Exception, match="float32"):
        attention_padded(hq, hk, hv, lens, 12)   # outside autocast nothing is cast behind the caller's back
