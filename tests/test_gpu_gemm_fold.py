"""The GEMM instances the encoder's fp16 fast mode dispatches -- the folded-LayerNorm epilogues EPI_RESLN (4), EPI_QK_F (5),
EPI_GELU_F (6) and EPI_VT_F (7) -- at hidden 768 and 1024, through ance_debug_gemm_hw, against the same expression in fp64 on the
same fp16 operands; and the N-split tile order (n_split = 2) of the epilogues the encoder runs with it.

The token operand is built the way the encoder holds it: a pre-LayerNorm row v travels as hi = fp16(v), lo = fp16(v - hi), and
its slice statistics (part_in: PartFormat of csrc/gemm_f16.h) are those of v itself.  Token rows have |mean| rstd of 0, 1.9, 2.1
and 30: the last two are WIDE (> FOLD_WIDE_MEAN = 2), so their tile runs the second K loop over the lo halves (masked to those
rows); they sit among ordinary rows in one tile, and another tile has none.  Needs an MI355X."""
import ctypes
import math

import pytest
import torch

from test_gpu_gemm import parts_of_rows, stats_of_parts

pytestmark = pytest.mark.gpu

U16 = 2.0 ** -11      # fp16 rounding of a stored output, relative
ACC = 3e-7            # fp32 accumulation and epilogue arithmetic, relative to the summed magnitudes (measured: <= 9.2e-8)
EPS = 1e-5
INTER = {768: 3072, 1024: 4096}
NAN16 = 0x7E5A        # the pattern an output is filled with before a launch (a quiet NaN)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def gemm_hw(epi, hw, **kw):
    """One launch of ance_debug_gemm_hw; keyword arguments are the fields of AnceGemmDebugArgs (tensors or plain values)."""
    from ance_amd import _lib
    L = _lib.lib()
    a = _lib.AnceGemmDebugArgs()
    a.scale = 1.0
    a.ln_eps = EPS
    for k, v in kw.items():
        setattr(a, k, _p(v) if isinstance(v, torch.Tensor) else v)
    rc = L.ance_debug_gemm_hw(epi, hw, ctypes.byref(a), _lib.current_stream_ptr())
    _lib.check(rc, "ance_debug_gemm_hw")
    torch.cuda.synchronize()


def _ratios(n):
    """|mean| rstd per token: 0 for most, 1.9 (ordinary, close to the threshold), 2.1 and 30 (wide) -- all in the first 256-token
    tile, mixed with ordinary rows; the second tile holds no wide token."""
    r = torch.zeros(n, dtype=torch.float64)
    for i in (9, 140, 300, 301, 400):
        r[i] = 1.9
    for i in (3, 77, 200):
        r[i] = 2.1
    for i in (5, 130, 255):
        r[i] = 30.0
    return r


def token_rows(n, hw, seed, ratios=None):
    """Pre-LayerNorm rows v [n, hw] (fp64) whose |mean| rstd is `ratios`, std between 0.5 and 2: (hi, lo, part_in, wide)."""
    g = torch.Generator().manual_seed(seed)
    ratios = _ratios(n) if ratios is None else ratios
    z = torch.randn((n, hw), generator=g, dtype=torch.float64)
    z = (z - z.mean(1, keepdim=True)) / z.std(1, unbiased=False, keepdim=True)
    sd = 0.5 + 1.5 * torch.rand(n, generator=g, dtype=torch.float64)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    mu = sign * ratios * torch.sqrt(sd ** 2 + EPS)
    v = (mu[:, None] + sd[:, None] * z).cuda()
    hi = v.half()
    lo = (v - hi.double()).half()
    part = parts_of_rows(v, hw)
    m, r = stats_of_parts(part, hw, EPS)
    wide = (m.abs() * r) > 2.0
    assert torch.equal(wide.cpu(), ratios > 2.0)
    return hi, lo, part, wide


def _weights(n, k, seed, scale=0.02):
    """A folded weight fp16(gamma W) [n, k], its row sums (csum, fp32) and a bias."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = torch.randn((n, k), generator=g, device="cuda", dtype=torch.float64) * scale
    gamma = 1.0 + 0.1 * torch.randn(k, generator=g, device="cuda", dtype=torch.float64)
    b = (w * gamma[None, :]).half()
    csum = b.double().sum(1).float()
    bias = (0.1 * torch.randn(n, generator=g, device="cuda", dtype=torch.float64)).float()
    return b, csum, bias


def _check(name, got, ref, scale, rel_out=U16, acc=ACC, extra=0.0, rows=None):
    """|got - ref| <= rel_out |ref| + acc scale + extra + 2^-24 on every element (of `rows` if given); returns the worst error in
    units of the accumulation term, printed."""
    if rows is not None:
        got, ref, scale = got[rows], ref[rows], scale[rows]
    err = (got - ref).abs()
    tol = rel_out * ref.abs() + acc * scale + extra + 2.0 ** -24
    bad = ~(err <= tol)
    worst = float(((err - rel_out * ref.abs() - extra).clamp_min(0) / scale).max()) if err.numel() else 0.0
    print("%s: max |err| %.3e, worst (|err| - output rounding) / scale %.3e (bound %.1e)" % (name, float(err.max()), worst, acc))
    assert not bad.any(), "%s: %d bad, max err %.4g at %s" % (name, int(bad.sum()), float(err.max()), torch.nonzero(bad)[:4].tolist())
    return worst


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _fold_ref(tok, w, csum, bias, part, hw, wide, lo=None):
    """r (tok_eff . w^T - mu csum) + bias in fp64 with tokens as ROWS: tok_eff = hi + lo on the wide rows when lo is given.
    Returns (ref, scale)."""
    m, r = stats_of_parts(part, hw, EPS)
    a = tok.double()
    if lo is not None:
        a = a + lo.double() * wide[:, None].double()
    acc = a @ w.double().t()
    ref = r[:, None] * (acc - m[:, None] * csum.double()[None, :]) + bias.double()[None, :]
    scale = r[:, None] * (a.abs() @ w.double().abs().t() + (m[:, None] * csum.double()[None, :]).abs()) + bias.double().abs()[None, :]
    return ref, scale


def _run_a_side(epi, hw, N, M=512, seed=0, tok_lo=True, scale_cols=0, qscale=1.0, ratios=None, n_split=0):
    """EPI_QK_F / EPI_GELU_F: tokens are the rows m.  Returns (got fp64 [M, N], hi, lo, part, wide, w, csum, bias)."""
    hi, lo, part, wide = token_rows(M, hw, seed, ratios)
    w, csum, bias = _weights(N, hw, seed + 1)
    out = torch.empty((M, N), dtype=torch.float16, device="cuda")
    out.view(torch.int16).fill_(NAN16)
    gemm_hw(epi, hw, a=hi, b=w, lda=hw, ldb=hw, M=M, N=N, K=hw, bias=bias, csum=csum, part_in=part, tok_lo=lo if tok_lo else None,
            scale=qscale, scale_cols=scale_cols, out=out, ldc=N, n_split=n_split)
    return out, hi, lo, part, wide, w, csum, bias


def _a_side_ref(epi, hw, hi, lo, part, wide, w, csum, bias, scale_cols=0, qscale=1.0):
    ref, scale = _fold_ref(hi, w, csum, bias, part, hw, wide, lo)
    if epi == 5:
        cs = torch.ones(w.shape[0], dtype=torch.float64, device="cuda")
        cs[:scale_cols] = qscale
        return ref * cs[None, :], scale * cs[None, :]
    return ref, scale


def _a_side_check(name, epi, hw, out, hi, lo, part, wide, w, csum, bias, used_lo, **kw):
    """Every row against the reference of the operand the kernel is meant to use (hi + lo on the wide rows when tok_lo was given,
    hi elsewhere); GELU: the exact erf form (the fp16 epilogue's gelu_erf256 documents |error| <= 8e-6 on [-9, 9], slope <= 1.13)."""
    ref, scale = _a_side_ref(epi, hw, hi, lo if used_lo else None, part, wide, w, csum, bias, **kw)
    got = out.double()
    if epi == 6:
        return _check(name, got, _gelu64(ref), 1.13 * scale, extra=8e-6), ref, scale
    return _check(name, got, ref, scale), ref, scale


@pytest.mark.parametrize("hw", [768, 1024])
@pytest.mark.parametrize("epi,what", [(5, "qk"), (5, "qk_split_tile"), (6, "ffn1")])
def test_folded_a_side_epilogues_against_fp64(hw, epi, what):
    """EPI_QK_F (Q | K projection, the scale on the Q columns < scale_cols) and EPI_GELU_F (FFN1) at the tower's shapes: K = hw,
    N = 2 hw / the intermediate size, two token tiles.  With tok_lo every row matches the operand it is meant to use -- the wide
    rows hi + lo, the ordinary ones hi -- and the hi-only reference is demonstrably outside the bound on the wide rows (the second
    K loop is needed and measured); without tok_lo every row is hi-only."""
    N = 2 * hw if epi == 5 else INTER[hw]
    kw = dict(scale_cols=hw if what == "qk" else 320, qscale=0.125 * 1.44269504088896340736) if epi == 5 else {}
    out, hi, lo, part, wide, w, csum, bias = _run_a_side(epi, hw, N, seed=hw + epi, **kw)
    name = "epi %d %s hw %d" % (epi, what, hw)
    _a_side_check(name + " tok_lo", epi, hw, out, hi, lo, part, wide, w, csum, bias, True, **kw)
    # the wide rows need their lo halves: the hi-only reference misses them by more than the bound
    ref0, scale0 = _a_side_ref(epi, hw, hi, None, part, wide, w, csum, bias, **kw)
    if epi == 6:
        ref0, scale0 = _gelu64(ref0), 1.13 * scale0
    err0 = ((out.double() - ref0).abs() - U16 * ref0.abs() - (8e-6 if epi == 6 else 0.0))[wide] / scale0[wide]
    print("%s: wide rows against the hi-only reference: worst %.3e" % (name, float(err0.max())))
    assert float(err0.max()) > 4 * ACC, float(err0.max())
    out2, *_ = _run_a_side(epi, hw, N, seed=hw + epi, tok_lo=False, **kw)
    _a_side_check(name + " no tok_lo", epi, hw, out2, hi, lo, part, wide, w, csum, bias, False, **kw)
    # ordinary rows never see the second loop: the same bits with and without tok_lo
    assert torch.equal(out.view(torch.int16)[~wide], out2.view(torch.int16)[~wide])


@pytest.mark.parametrize("hw", [768, 1024])
@pytest.mark.parametrize("epi", [5, 6])
def test_folded_a_side_rows_do_not_depend_on_their_tile_mates(hw, epi):
    """The second K loop is masked per token row: an ordinary row's output bits are the same whether or not a wide row shares its
    tile (here the wide rows of the first tile are replaced by ordinary ones, so that tile runs no second loop at all)."""
    N = 2 * hw if epi == 5 else INTER[hw]
    kw = dict(scale_cols=hw, qscale=0.125) if epi == 5 else {}
    a, _, _, _, wide, *_ = _run_a_side(epi, hw, N, seed=7 + hw, **kw)
    calm = _ratios(512)
    calm[calm > 2] = 0.0
    b, *_ = _run_a_side(epi, hw, N, seed=7 + hw, ratios=calm, **kw)
    assert wide.any()
    assert torch.equal(a.view(torch.int16)[~wide], b.view(torch.int16)[~wide])


def _vt_layout(n_tok, n_valid, seed):
    """col_map of V^T: sequences of random lengths, each starting at an 8-aligned column with an 8-column gap before it; tokens
    >= n_valid map (in range) into the gaps.  Returns (col_map int32 [n_tok], ldc, the mapped columns of the valid tokens)."""
    g = torch.Generator().manual_seed(seed)
    cols, c, t = [], 0, 0
    gaps = []
    while t < n_valid:
        ln = min(int(torch.randint(1, 140, (1,), generator=g)), n_valid - t)
        gaps += list(range(c, c + 8))
        c += 8
        cols += list(range(c, c + ln))
        c = (c + ln + 7) // 8 * 8
        t += ln
    ldc = c + 64
    gaps += list(range(c, ldc))
    cols += [gaps[i % len(gaps)] for i in range(n_tok - n_valid)]
    return torch.tensor(cols, dtype=torch.int32, device="cuda"), ldc


def _run_vt(hw, n_tok, n_valid, seed, tok_lo=True, ratios=None):
    hi, lo, part, wide = token_rows(n_tok, hw, seed, ratios)
    w, csum, bias = _weights(hw, hw, seed + 1)           # the value projection: features x K
    col_map, ldc = _vt_layout(n_tok, n_valid, seed)
    out = torch.empty((hw, ldc), dtype=torch.float16, device="cuda")
    out.view(torch.int16).fill_(NAN16)
    gemm_hw(7, hw, a=w, b=hi, lda=hw, ldb=hw, M=hw, N=n_tok, K=hw, bias=bias, csum=csum, part_in=part, tok_lo=lo if tok_lo else None,
            col_map=col_map, n_valid=n_valid, out=out, ldc=ldc)
    return out, hi, lo, part, wide, w, csum, bias, col_map


@pytest.mark.parametrize("hw", [768, 1024])
def test_folded_vt_epilogue_against_fp64(hw):
    """EPI_VT_F (V^T = Wv h^T, tokens are the B-operand rows and the output COLUMNS): three token tiles with n_valid < N, scattered
    through a col_map with 8-aligned gaps between the sequences.  The columns of valid tokens match fp64 (wide tokens with their
    lo halves when tok_lo is given, hi-only without it); every other column keeps the NaN pattern it was filled with; the tokens
    >= n_valid (mapped into the gaps) are not stored."""
    n_tok, n_valid = 768, 700
    out, hi, lo, part, wide, w, csum, bias, col_map = _run_vt(hw, n_tok, n_valid, seed=hw + 70)
    cm = col_map[:n_valid].long()
    untouched = torch.ones(out.shape[1], dtype=torch.bool, device="cuda")
    untouched[cm] = False
    assert int(untouched.sum()) > 0 and bool((out.view(torch.int16)[:, untouched] == NAN16).all()), "V^T wrote outside its columns"
    for used_lo, o in ((True, out), (False, _run_vt(hw, n_tok, n_valid, seed=hw + 70, tok_lo=False)[0])):
        ref, scale = _fold_ref(hi, w, csum, bias, part, hw, wide, lo if used_lo else None)   # [tokens, features]
        got = o.double()[:, cm].t()
        _check("epi 7 hw %d %s" % (hw, "tok_lo" if used_lo else "no tok_lo"), got, ref[:n_valid], scale[:n_valid])
        assert bool((o.view(torch.int16)[:, untouched] == NAN16).all())
    ref0, scale0 = _fold_ref(hi, w, csum, bias, part, hw, wide, None)
    wv = wide[:n_valid]
    err0 = ((out.double()[:, cm].t() - ref0[:n_valid]).abs() - U16 * ref0[:n_valid].abs())[wv] / scale0[:n_valid][wv]
    print("epi 7 hw %d: wide tokens against the hi-only reference: worst %.3e" % (hw, float(err0.max())))
    assert float(err0.max()) > 4 * ACC


@pytest.mark.parametrize("hw", [768, 1024])
def test_folded_vt_tokens_do_not_depend_on_their_tile_mates(hw):
    """The B-side form of the masked second K loop: an ordinary token's V^T column has the same bits whether or not wide tokens
    share its tile."""
    a, _, _, _, wide, _, _, _, col_map = _run_vt(hw, 768, 700, seed=hw + 71)
    calm = _ratios(768)
    calm[calm > 2] = 0.0
    b = _run_vt(hw, 768, 700, seed=hw + 71, ratios=calm)[0]
    keep = col_map[:700][~wide[:700]].long()
    assert wide[:700].any() and torch.equal(a.view(torch.int16)[:, keep], b.view(torch.int16)[:, keep])


@pytest.mark.parametrize("hw", [768, 1024])
@pytest.mark.parametrize("k_of", ["hw", "inter"])
def test_resln_epilogue_against_fp64(hw, k_of):
    """EPI_RESLN (attention.output.dense / output.dense + residual LayerNorm): acc + bias + LayerNorm(res_hi + res_lo) stored as a
    (hi, lo) pair -- 22 bits: 2^-22 of the value on top of the accumulation term -- and part_out, the output rows' slice
    statistics in the hidden width's format (twelve 64-column slices at 768, eight 128-column slices at 1024, the last 8 of the
    24 floats untouched)."""
    M, N = 512, hw
    K = hw if k_of == "hw" else INTER[hw]
    g = torch.Generator(device="cuda").manual_seed(hw + K)
    a = (torch.randn((M, K), generator=g, device="cuda") * 0.5).half()
    w, _, bias = _weights(N, K, hw + K + 1)
    rhi, rlo, part, _ = token_rows(M, hw, hw + K + 2)
    gamma = 1.0 + 0.2 * torch.randn(N, generator=g, device="cuda")
    beta = 0.1 * torch.randn(N, generator=g, device="cuda")
    hi = torch.empty((M, N), dtype=torch.float16, device="cuda")
    lo = torch.empty_like(hi)
    hi.view(torch.int16).fill_(NAN16)
    lo.view(torch.int16).fill_(NAN16)
    part_out = torch.full((M, 24), float("nan"), device="cuda")
    gemm_hw(4, hw, a=a, b=w, lda=K, ldb=K, M=M, N=N, K=K, bias=bias, part_in=part, res_hi=rhi, res_lo=rlo, res_gamma=gamma,
            res_beta=beta, out=hi, out_lo=lo, part_out=part_out, ldc=N)
    m, r = stats_of_parts(part, hw, EPS)
    R = rhi.double() + rlo.double()
    ref = a.double() @ w.double().t() + bias.double()[None, :] + (R - m[:, None]) * r[:, None] * gamma.double()[None, :] + beta.double()[None, :]
    scale = a.double().abs() @ w.double().abs().t() + bias.double().abs()[None, :] + \
        (R.abs() + m.abs()[:, None]) * r[:, None] * gamma.double().abs()[None, :] + beta.double().abs()[None, :]
    got = hi.double() + lo.double()
    _check("epi 4 hw %d K %d" % (hw, K), got, ref, scale, rel_out=2.0 ** -22)
    # slice means: the split tests' 2e-6 plus the outputs' accumulation term averaged over the slice (the residual rows with a
    # large mean cancel r gamma res against r gamma mean in fp32); M2: the split tests' 2e-5 relative
    want = parts_of_rows(ref, hw)
    ns = 12 if hw == 768 else 8
    pm, pq = part_out[:, 0:2 * ns:2].double(), part_out[:, 1:2 * ns:2].double()
    wm, wq = want[:, 0:2 * ns:2].double(), want[:, 1:2 * ns:2].double()
    sm = scale.reshape(M, ns, -1).mean(-1)
    dm, dq = (pm - wm).abs(), (pq - wq).abs() / wq
    print("epi 4 hw %d K %d part_out: max |d mean| %.3e (%.3e of its bound), max rel d M2 %.3e" % (
        hw, K, float(dm.max()), float((dm / (2e-6 + ACC * sm)).max()), float(dq.max())))
    assert bool((dm <= 2e-6 + ACC * sm).all()) and float(dq.max()) <= 2e-5, (float(dm.max()), float(dq.max()))
    assert bool(torch.isnan(part_out[:, 2 * ns:]).all()), "part_out written past the hidden width's slices"


@pytest.mark.parametrize("hw", [768, 1024])
@pytest.mark.parametrize("epi,stream", [(6, "1"), (9, "1"), (9, "0")])   # (ANCE_GEMM_STREAM selects among the split kernels only)
def test_n_split_tile_order_changes_no_bit(hw, epi, stream, monkeypatch):
    """FFN1 runs with n_split = 2 (the N-split tile order of gemm256_tile.h: tile_of_block) in both fp16 (EPI_GELU_F) and split
    (EPI_S_GELU: the streaming kernel and the launch-per-tile kernel) modes: the same output bits as the plain order, on a token
    count that is not a multiple of four tiles (the padded grid of the N-split order)."""
    from ance_amd import _lib
    from test_gpu_gemm import _pair, _pair_rows
    M, N, K = 1280, INTER[hw], hw
    monkeypatch.setenv("ANCE_GEMM_STREAM", stream)
    _lib.reload_env()
    try:
        outs = []
        for ns in (2, 0):
            if epi == 6:
                outs.append(_run_a_side(6, hw, N, M=M, seed=hw + 90, ratios=_ratios(M), n_split=ns)[0])
                continue
            hi, lo, part, _ = token_rows(M, hw, hw + 91)
            ap = _pair_rows(*_pair(hi.float() + lo.float()))
            w, csum, bias = _weights(N, K, hw + 92, scale=0.02 * 2.0 ** 13)
            bp = _pair_rows(*_pair(w.float()))
            winv = torch.tensor([2.0 ** -13], device="cuda")
            out = torch.zeros((M, 2 * N), dtype=torch.float16, device="cuda")
            gemm_hw(9, hw, a=ap, b=bp, lda=2 * K, ldb=2 * K, M=M, N=N, K=K, bias=bias, csum=csum * 2.0 ** -13, part_in=part, out=out,
                    ldc=2 * N, wscale_inv=winv, n_split=ns)
            outs.append(out)
    finally:
        monkeypatch.delenv("ANCE_GEMM_STREAM", raising=False)
        _lib.reload_env()
    assert bool(torch.isfinite(outs[0].float()).all())
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), (hw, epi, stream)
