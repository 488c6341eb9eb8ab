"""The split GEMM's main loop on v_mfma_f32_16x16x32_f16 (csrc/pipe256.h, PAIR3), through the C-ABI test hook with the fp32
epilogue set up so that its output IS the accumulator (mean 0, rstd 1, csum 0, bias 0):
  * one-hot A rows: row m of A holds a single 1 at k = k_m (in its hi half, or in its lo half), so out[m][n] must equal exactly one
    element of B (B_hi + B_lo, or B_hi) -- every (m, n) and every position inside the 32-deep k-blocks is checked bit for bit, which
    the tolerance tests of tests/test_gpu_gemm.py cannot do for a k that is permuted inside a block;
  * the rounding bias of the accumulation against fp64 at K = 768 and 3 x 768: the scheme is fp32-grade only if the fp16 MFMA
    accumulates with round-to-nearest.  Needs an MI355X."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def _pair_rows(hi, lo):
    """(hi, lo) [R, W] fp16 -> pair rows [R, 2 W] at the positions the library reports (ance_pair_layout)"""
    from ance_amd import _lib
    L = _lib.lib()
    R, W = hi.shape
    h, l, sc = ctypes.c_int(), ctypes.c_int(), ctypes.c_float()
    hc, lc = [], []
    for n in range(W):
        L.ance_pair_layout(n, W, ctypes.byref(h), ctypes.byref(l), ctypes.byref(sc))
        hc.append(h.value)
        lc.append(l.value)
    assert sc.value == 1.0
    out = torch.zeros((R, 2 * W), dtype=torch.float16, device=hi.device)
    out[:, torch.tensor(hc, device=hi.device)] = hi
    out[:, torch.tensor(lc, device=hi.device)] = lo
    return out.contiguous()


def _acc(ah, al, bh, bl):
    """the raw accumulator sum_k ah bh + al bh + ah bl [M, N] fp32, from ance_debug_gemm_split epilogue 8 with r = 1, mu = 0"""
    from ance_amd import _lib
    L = _lib.lib()
    M, K = ah.shape
    N = bh.shape[0]
    ap, bp = _pair_rows(ah, al), _pair_rows(bh, bl)
    zeros = torch.zeros(N, device="cuda")
    part = torch.zeros((M, 12, 2), device="cuda")
    part[:, :, 1] = 64.0  # twelve 64-column slices of mean 0 and variance 1 -> mu = 0, r = 1 (ln_eps 0)
    out = torch.empty((M, N), device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.ance_debug_gemm_split(8, P(ap), P(bp), M, N, K, P(zeros), P(zeros), None, P(part), 0.0, None, P(out), None, None,
                                 _lib.current_stream_ptr())
    _lib.check(rc, "ance_debug_gemm_split")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("half", ["hi", "lo"])
@pytest.mark.parametrize("shape", [(768, 512, 768), (256, 256, 3072)])
def test_one_hot_rows_pick_one_k(half, shape):
    M, N, K = shape
    g = torch.Generator(device="cuda").manual_seed(3)
    m = torch.arange(M, device="cuda")
    km = (m * 37 + (m // K) * 5) % K  # 37 is prime to K: distinct k for K consecutive rows, every position of every 32-deep block
    one = torch.zeros((M, K), dtype=torch.float16, device="cuda")
    one[m, km] = 1.0
    zero = torch.zeros_like(one)
    ah, al = (one, zero) if half == "hi" else (zero, one)
    b = torch.randn((N, K), generator=g, device="cuda")
    bh = b.half()
    bl = (b - bh.float()).half()
    got = _acc(ah, al, bh, bl)
    # hi: hi x hi + hi x lo = B_hi + B_lo (exact in fp32: 22 bits);  lo: lo x hi = B_hi
    want = (bh.float() + bl.float())[:, km].t() if half == "hi" else bh.float()[:, km].t()
    bad = got != want
    assert not bool(bad.any()), (half, shape, int(bad.sum()), torch.nonzero(bad)[:4].tolist())


def _ulp32(x):
    return torch.ldexp(torch.ones_like(x), (torch.frexp(x.abs().clamp_min(1e-30))[1] - 24).int())


@pytest.mark.parametrize("K", [768, 2304])
def test_accumulation_is_unbiased(K):
    """All-positive pair operands (partial sums grow monotonically: a truncating accumulator would be off by about half an ulp per
    K-step of 32, i.e. -10 ulp and more here); the mean signed error over 786,432 outputs in units of the result's fp32 ulp.
    The matrix core leaves a small negative bias on such chains: -0.17 ulp at K = 768 and -0.84 at K = 2,304, and the 32x32x16
    form measured the same (-0.16 / -0.84 on the same data, profiles/r07_accumulation_bias.txt).  The bound, 0.5 ulp per 768 of K,
    keeps that and rejects truncation by a factor of 20."""
    M, N = 1024, 768
    g = torch.Generator(device="cuda").manual_seed(5)
    a = torch.randn((M, K), generator=g, device="cuda").abs() + 1.0
    b = torch.randn((N, K), generator=g, device="cuda").abs() * 0.02 + 0.01
    ah, bh = a.half(), b.half()
    al, bl = (a - ah.float()).half(), (b - bh.float()).half()
    got = _acc(ah, al, bh, bl).double()
    Ah, Al, Bh, Bl = ah.double(), al.double(), bh.double(), bl.double()
    exact = Ah @ Bh.t() + Al @ Bh.t() + Ah @ Bl.t()
    err = (got - exact) / _ulp32(exact)
    mean = float(err.mean())
    print("K %d: mean signed error %+.4f ulp, std %.3f, max |err| %.2f" % (K, mean, float(err.std()), float(err.abs().max())))
    assert abs(mean) <= 0.5 * K / 768, (K, mean, float(err.std()), float(err.abs().max()))
    assert float(err.abs().max()) < 24.0 * K / 768, (K, float(err.abs().max()))
