"""The encoder's three attention kernels -- attention_kernel<4> (fp16 fast mode, kind 0), attention_split_kernel<4> (the default split
mode, kind 1) and attention32_kernel<768|1024> (fp32 audit mode, kind 2) -- through ance_debug_attention, against softmax attention
in fp64 on the exact operand values each kernel reads:

    o = sum_j w_j v_j,  w = softmax(s);  kind 0: s_j = sum_d q_d k_jd in the log2 domain (Q stored pre-scaled by log2(e) / 8 and
    rounded to fp16, as the EPI_QK_F epilogue delivers it), w ~ 2^s;  kinds 1, 2: s_j = (q . k_j) / 8 on the fp32 values, w ~ e^s.

Bounds, per output element, from the arithmetic (U = 2^-24; A = sum_j w_j |v_j|; D = max_j v_j - min_j v_j >= max |v_j - o| per
head dim; E = max_j sum_d |q_d k_jd| in natural score units; Sv = sum_j |v_j| / sum_j e^(s_j - max s); nkb = ceil(T / 32)).  A
relative error eps_j of the weight of key j moves o by at most 2 max|eps| D; eps_j = ln2 times the log2-domain score error, which
is a count of roundings of E, plus the exp error (v_exp_f32 / expf: <= 2 ulp, shared by numerator and l, so it enters through D):
  kind 0  P is rounded to fp16 for the numerator only (l sums the fp32 P): 2^-11 A, and 2^-25 absolute for each P below 2^-14 (the
          fp16 subnormal spacing), divided by l: 2^-25 Sv; the output store 2^-11 |o|; the fp32 MFMA accumulation (2 per key block),
          the rescales and the l sum: (2 nkb + 8) U A + (nkb + 24) U |o|; scores (fp16 operands exact, fp32 sums, s - m): <= 8 U E
          per score -> 16 U E D; exp: 8 U D; 2^-25 absolute (fp16 subnormal output).
  kind 1  operands v = hi + lo' 2^-11 carry 2^-22 of |v| each; the dropped lo' x lo' products another 2^-22: 3 2^-22 A on the
          numerator, and about 12 U of E on a score (+ qscale rounded to fp32, the MFMA chain of 12 products, s - m: <= 24 U E,
          48 U E D); accumulation (4 nkb + 16) U A, l and the final fma / scale (nkb + 24) U |o|; the pair store 2^-22 |o| + 2^-25;
          P and V below the lo' normal range: 2^-36 Sv; a Q or K element whose lo' is subnormal (Q of the +-65504 regime, whose hi is
          itself an fp16 subnormal) is off by up to 2^-36 absolute: 2^-35 (max_j sum_d |k_jd| + sum_d |q_d|) D.
  kind 2  the sequential fmaf chains: (2 T + 8) U A (one product and one fma rounding per key, each at most U of the running sum of
          |w v|), (T + 8) U |o| (lsum, the final scale), a 64-term fmaf score chain and s - m: <= 66 U E per score -> 132 U E D.
Measured worst fraction of these bounds over every case here (each test prints its worst element and the terms there; MI355X):
kind 0 0.73 (the fp16 rounding of P and of the output), kind 1 0.85 (at T = 1, where the 2^-25 of the pair store's fp16-subnormal
lo half is the whole bound), kind 2 0.08.  A stored pair has |lo| <= ulp(hi) / 2 and hi a nearest fp16 of hi + lo (checked on
every element).

Every buffer a kernel must not read or write holds the NaN pattern: token rows between sequences and 160 guard rows after the last,
the V^T columns outside [vcol, vcol + T) (the gap columns up to roundup8(T) included), the Q columns of every row that is no
sequence's compact row under q_compact, and all of ctx before the launch.  Afterwards the inputs are bit for bit unchanged and every
ctx element no sequence owns is still the pattern.  The bit identities the encoder relies on -- a sequence's output does not depend on
its batch mates, the descriptor order, its tok0 / vcol, the launch's max_seq_len or the head count; cls_only (+ q_compact) reproduces
row tok0 of the full launch -- are checked bit for bit.  Needs an MI355X."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN16 = 0x7E5A        # fp16 quiet NaN: the pattern of every element a kernel must not read or write
NAN32 = 0x7FC07E5A    # its fp32 counterpart
LOG2E = 1.4426950408889634
U = 2.0 ** -24
GUARD = 160           # NaN rows after the last sequence: more than any over-read of a 128-key chunk or a 32-key block
LENGTHS = (1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 287, 288, 289, 383, 384, 511, 512)
HEADS = (12, 16)
KINDS = (0, 1, 2)


class Layout:
    """Token rows and V^T columns of a launch: sequence s owns rows tok0[s] .. + len and V^T columns vcol[s] .. + len (8-aligned).
    gaps: 1-4 NaN rows between sequences (kinds 0, 1; the fp32 kernel's seq_off packs them) and 8-16 NaN columns between their V^T
    blocks; `first` rows before the first sequence."""

    def __init__(self, lens, kind, seed, gaps=True, first=None):
        rng = np.random.default_rng(seed)
        self.lens = [int(t) for t in lens]
        self.kind = kind
        t = int(rng.integers(1, 7)) if first is None else first
        c = 8 * int(rng.integers(1, 3)) if gaps else 0
        self.tok0, self.vcol = [], []
        for T in self.lens:
            self.tok0.append(t)
            self.vcol.append(c)
            t += T + (int(rng.integers(1, 5)) if gaps and kind != 2 else 0)
            c += (T + 7) // 8 * 8 + (8 * int(rng.integers(1, 3)) if gaps else 0)
        self.rows = t + GUARD
        self.vt_cols = c + 64
        # plan_kernel's order: length buckets ceil(len / 32) - 1 capped at 3, longest bucket first, then the sequence index
        bucket = [min((T + 31) // 32 - 1, 3) for T in self.lens]
        self.order = sorted(range(len(self.lens)), key=lambda s: (-bucket[s], s))

    def desc(self, order=None):
        if self.kind == 2:
            return np.array(self.tok0 + [self.tok0[-1] + self.lens[-1]], dtype=np.int32)
        order = self.order if order is None else order
        return np.array([[self.tok0[s], self.lens[s], self.vcol[s], s] for s in order], dtype=np.int32)


def _nan(shape, dtype):
    if dtype == torch.float16:
        return torch.full(shape, NAN16, dtype=torch.int16, device="cuda").view(torch.float16)
    return torch.full(shape, NAN32, dtype=torch.int32, device="cuda").view(torch.float32)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.float16 else t.view(torch.int32)


def _is_nan_pattern(t):
    return _bits(t) == (NAN16 if t.dtype == torch.float16 else NAN32)


class Bufs:
    """kind 0: qk fp16 [rows, ld_qk] = fp16(q log2(e) / 8) | fp16(k), vt fp16 [H, ld_vt], ctx fp16 [rows, ld_ctx];
    kinds 1, 2: qk fp32 [rows, 3 H] = q | k | v; ctx fp16 pair rows [rows, 2 H] (kind 1) or fp32 [rows, H] (kind 2).
    pad: extra columns of the kind-0 row strides (NaN, never touched)."""

    def __init__(self, kind, nh, lay, pad=0):
        H = 64 * nh
        self.kind, self.nh, self.H, self.lay = kind, nh, H, lay
        self.vt = None
        if kind == 0:
            self.qk = _nan((lay.rows, 2 * H + pad), torch.float16)
            self.vt = _nan((H, lay.vt_cols + pad), torch.float16)
            self.ctx = _nan((lay.rows, H + pad), torch.float16)
        else:
            self.qk = _nan((lay.rows, 3 * H), torch.float32)
            self.ctx = _nan((lay.rows, 2 * H), torch.float16) if kind == 1 else _nan((lay.rows, H), torch.float32)

    def put(self, s, q, k, v):
        """q, k, v fp64 [T, nh, 64] of sequence s, natural scores (q . k) / 8"""
        t0, T, H = self.lay.tok0[s], self.lay.lens[s], self.H
        q, k, v = (x[:, :self.nh].reshape(T, H) for x in (q, k, v))
        if self.kind == 0:
            self.qk[t0:t0 + T, :H] = (q * (LOG2E / 8.0)).half()
            self.qk[t0:t0 + T, H:2 * H] = k.half()
            c0 = self.lay.vcol[s]
            self.vt[:, c0:c0 + T] = v.t().half()
        else:
            self.qk[t0:t0 + T] = torch.cat([q, k, v], 1).float()

    def fresh_ctx(self):
        self.ctx = _nan(tuple(self.ctx.shape), self.ctx.dtype)


def launch(b, desc, max_seq_len=512, cls_only=0, q_compact=0):
    from ance_amd import _lib
    L = _lib.lib()
    d = np.ascontiguousarray(desc, dtype=np.int32)
    dd = torch.empty(d.size + 4, dtype=torch.int32, device="cuda")
    a = _lib.AnceAttnDebugArgs(kind=b.kind, n_heads=b.nh, n_seq=len(d) - 1 if b.kind == 2 else len(d), max_seq_len=max_seq_len,
                               cls_only=cls_only, q_compact=q_compact, h_desc=d.ctypes.data, d_desc=dd.data_ptr(),
                               d_desc_bytes=dd.numel() * 4, qk=b.qk.data_ptr(), ld_qk=b.qk.stride(0), qk_rows=b.qk.shape[0],
                               vt=b.vt.data_ptr() if b.vt is not None else None, ld_vt=b.vt.stride(0) if b.vt is not None else 0,
                               ctx=b.ctx.data_ptr(), ld_ctx=b.ctx.stride(0), ctx_rows=b.ctx.shape[0])
    rc = L.ance_debug_attention(ctypes.byref(a), _lib.current_stream_ptr())
    _lib.check(rc, "ance_debug_attention")
    torch.cuda.synchronize()


# ---- operands ---------------------------------------------------------------------------------------------------------------------

def seq_data(T, nh, spec, g):
    """q, k, v fp64 [T, nh, 64] (natural scores (q . k) / 8) of one regime:
    ("ord",)          N(0, 1) rows
    ("flat",)         one key row repeated: o = the mean of V over exactly T keys
    ("sat", p, q0)    key p scores ~48 (>= 30 checked) above every other key for the queries >= q0; for the others it is ordinary
    ("wide",)         scores spread over [-41, 0] (log2 domain [-60, 0]): fp16 P subnormal and zero in kind 0
    ("mean",)         V = 300 + N(0, 1)
    ("range",)        K, V uniform in [-65504, 65504] with exact +-65504 entries (RANGE_LIMIT), Q ~ 1e-4"""
    rn = lambda *sh: torch.randn(sh, generator=g, device="cuda", dtype=torch.float64)  # noqa: E731
    name = spec[0]
    if name in ("ord", "mean"):
        q, k, v = rn(T, nh, 64), rn(T, nh, 64), rn(T, nh, 64)
        return q, k, (v + 300.0 if name == "mean" else v)
    if name == "flat":
        return rn(T, nh, 64), rn(1, nh, 64).expand(T, nh, 64).clone(), rn(T, nh, 64)
    if name == "range":
        uni = lambda: (torch.rand((T, nh, 64), generator=g, device="cuda", dtype=torch.float64) * 2 - 1) * 65504.0  # noqa: E731
        k, v = uni(), uni()
        k[::7, :, 3] = 65504.0
        k[1::5, :, 9] = -65504.0
        v[::5, :, 7] = -65504.0
        v[2::3, :, 60] = 65504.0
        return 1e-4 * rn(T, nh, 64), k, v
    u = rn(nh, 64)
    u = u / u.norm(dim=-1, keepdim=True)
    orth = lambda x: x - (x * u).sum(-1, keepdim=True) * u  # noqa: E731
    if name == "sat":
        p, q0 = spec[1], spec[2]
        a = torch.zeros((T, 1, 1), device="cuda", dtype=torch.float64)
        a[q0:] = 4.0
        q = orth(0.3 * rn(T, nh, 64)) + a * u
        k = orth(rn(T, nh, 64))
        k[p] = 96.0 * u
        return q, k, rn(T, nh, 64)
    assert name == "wide"
    c = torch.rand((T, nh, 1), generator=g, device="cuda", dtype=torch.float64) * 83.0
    return orth(0.3 * rn(T, nh, 64)) + 4.0 * u, orth(0.5 * rn(T, nh, 64)) - c * u, rn(T, nh, 64)


def fill(b, specs, seed, datas=None):
    g = torch.Generator(device="cuda").manual_seed(seed)
    for s, T in enumerate(b.lay.lens):
        b.put(s, *(datas[s] if datas is not None else seq_data(T, b.nh, specs[s], g)))


def operands(b, s, q_row=None):
    """q [Tq, nh, 64], k, v [T, nh, 64] fp64 as the kernel reads them, q in natural score units (scores = q . k)"""
    t0, T, H, nh = b.lay.tok0[s], b.lay.lens[s], b.H, b.nh
    rows = slice(t0, t0 + T) if q_row is None else slice(q_row, q_row + 1)
    if b.kind == 0:
        q = b.qk[rows, :H].double() * math.log(2.0)
        k = b.qk[t0:t0 + T, H:2 * H].double()
        c0 = b.lay.vcol[s]
        v = b.vt[:, c0:c0 + T].t().double()
    else:
        q = b.qk[rows, :H].double() / 8.0
        k = b.qk[t0:t0 + T, H:2 * H].double()
        v = b.qk[t0:t0 + T, 2 * H:3 * H].double()
    return q.reshape(-1, nh, 64), k.reshape(T, nh, 64), v.reshape(T, nh, 64)


def reference(kind, q, k, v):
    """(o, tol, s) in fp64: o, tol [Tq, nh, 64] (the module docstring's bound), s [nh, Tq, T] natural scores"""
    qh, kh, vh = (x.permute(1, 0, 2) for x in (q, k, v))
    s = qh @ kh.transpose(1, 2)
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    lsum = e.sum(-1, keepdim=True)
    w = e / lsum
    o = w @ vh
    A = w @ vh.abs()
    E = (qh.abs() @ kh.abs().transpose(1, 2)).max(-1, keepdim=True).values
    D = vh.max(1, keepdim=True).values - vh.min(1, keepdim=True).values
    Sv = vh.abs().sum(1, keepdim=True) / lsum
    KQ = kh.abs().sum(-1).max(-1).values[:, None, None] + qh.abs().sum(-1, keepdim=True)  # max_j sum_d |k_jd| + sum_d |q_d|
    T = k.shape[0]
    nkb = (T + 31) // 32
    cKQ = 0.0
    if kind == 0:
        cA, co, cE, cS, cabs = 2.0 ** -11 + (2 * nkb + 8) * U, 2.0 ** -11 + (nkb + 24) * U, 16 * U, 2.0 ** -25, 2.0 ** -25
    elif kind == 1:
        cA, co, cE, cS, cabs = 3 * 2.0 ** -22 + (4 * nkb + 16) * U, 2.0 ** -22 + (nkb + 24) * U, 48 * U, 2.0 ** -36, 2.0 ** -25
        cKQ = 2.0 ** -35
    else:
        cA, co, cE, cS, cabs = (2 * T + 8) * U, (T + 8) * U, 132 * U, 0.0, 2.0 ** -60
    terms = (cA * A, co * o.abs(), (cE * E + cKQ * KQ + 8 * U) * D, cS * Sv + cabs)
    tol = terms[0] + terms[1] + terms[2] + terms[3]
    return o.permute(1, 0, 2), tol.permute(1, 0, 2), s, [t.expand_as(o).permute(1, 0, 2) for t in terms]


@functools.lru_cache(maxsize=None)
def _pair_cols(W):
    from ance_amd import _lib
    L = _lib.lib()
    hi, lo, sc = ctypes.c_int(), ctypes.c_int(), ctypes.c_float()
    hc, lc = [], []
    for n in range(W):
        L.ance_pair_layout(n, W, ctypes.byref(hi), ctypes.byref(lo), ctypes.byref(sc))
        hc.append(hi.value)
        lc.append(lo.value)
    return torch.tensor(hc, device="cuda"), torch.tensor(lc, device="cuda"), float(sc.value)


def output(b, rows):
    """ctx rows -> fp64 [len(rows), nh, 64]; kind 1: decodes the pair rows and checks hi == fp16(hi + lo), |lo| <= ulp(hi) / 2 on
    every element"""
    H = b.H
    r = b.ctx[rows]
    if b.kind == 1:
        hc, lc, sc = _pair_cols(H)
        hi, lo = r[:, hc], r[:, lc].float() / sc
        ulp = torch.exp2(torch.floor(torch.log2(hi.double().abs().clamp_min(2.0 ** -14))) - 10)
        assert bool((lo.double().abs() <= ulp / 2).all()), "pair: |lo| > ulp(hi) / 2"
        # hi is a nearest fp16 of hi + lo: fp16(hi + lo) == hi, or hi + lo is a tie (|lo| = ulp / 2 exactly -- lo = fp16(v - hi) is
        # itself rounded, so a v - hi just inside half an ulp can land on it, and the tie of hi + lo may then break the other way)
        nearest = (_bits((hi.float() + lo).half()) == _bits(hi)) | (lo.double().abs() == ulp / 2)
        assert bool(nearest.all()), "pair: hi is not a nearest fp16 of hi + lo (%d elements)" % int((~nearest).sum())
        out = hi.double() + lo.double()
    else:
        out = r[:, :H].double()
    return out.reshape(-1, b.nh, 64)


def check(b, seqs=None, cls=False, compact=False, name=""):
    """Every output of sequences `seqs` (all) against fp64; returns the worst fraction of the bound"""
    worst, worst_at = 0.0, ""
    for s in (range(len(b.lay.lens)) if seqs is None else seqs):
        t0 = b.lay.tok0[s]
        q, k, v = operands(b, s, q_row=(s if compact else t0) if cls else None)
        o, tol, _, terms = reference(b.kind, q, k, v)
        got = output(b, [s] if cls else slice(t0, t0 + b.lay.lens[s]))
        err = (got - o).abs()
        bad = ~(err <= tol)
        frac = err / tol
        i = int(frac.argmax())
        where = "seq %d (T=%d) at %s: err %.3g = %.3g of the bound; terms A %.3g, |o| %.3g, D %.3g, abs %.3g" % (
            s, b.lay.lens[s], list(np.unravel_index(i, tuple(frac.shape))), float(err.flatten()[i]), float(frac.flatten()[i]),
            *(float(t.flatten()[i]) for t in terms))
        assert not bad.any(), "%s kind %d: %d bad; worst %s" % (name, b.kind, int(bad.sum()), where)
        if float(frac.max()) > worst:
            worst, worst_at = float(frac.max()), where
    print("%s kind %d, %d heads: worst |err| / bound %.3g, %s" % (name, b.kind, b.nh, worst, worst_at))
    return worst


def check_isolation(b, before, out_rows):
    """inputs unchanged; ctx: the rows out_rows (columns [0, H), kind 1 [0, 2 H)) finite, every other element the NaN pattern"""
    assert torch.equal(_bits(b.qk), _bits(before[0])), "the kernel wrote into its Q | K (| V) input"
    if b.vt is not None:
        assert torch.equal(_bits(b.vt), _bits(before[1])), "the kernel wrote into V^T"
    owned = torch.zeros(b.ctx.shape, dtype=torch.bool, device="cuda")
    width = 2 * b.H if b.kind == 1 else b.H
    owned[torch.as_tensor(out_rows, device="cuda", dtype=torch.long), :width] = True
    nanp = _is_nan_pattern(b.ctx)
    assert bool(nanp[~owned].all()), "ctx written outside the sequences' rows: %s" % torch.nonzero(~nanp & ~owned)[:4].tolist()
    assert bool(torch.isfinite(b.ctx[owned].float()).all()), "non-finite output"


def _rows(lay, seqs=None):
    return [r for s in (range(len(lay.lens)) if seqs is None else seqs) for r in range(lay.tok0[s], lay.tok0[s] + lay.lens[s])]


def _snapshot(b):
    return b.qk.clone(), (b.vt.clone() if b.vt is not None else None)


# ---- tests ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nh", HEADS)
@pytest.mark.parametrize("kind", KINDS)
def test_every_length_against_fp64(kind, nh):
    """All 24 lengths (every partial 32-key block, the 128-query pass, the 256-key chunk of the split kernel, the 128-key chunk and
    256-query round of the fp32 kernel) mixed in one launch with NaN gaps and guard rows; kind 0 also with padded row strides."""
    lay = Layout(LENGTHS, kind, seed=1)
    b = Bufs(kind, nh, lay, pad=24 if kind == 0 else 0)
    fill(b, [("ord",)] * len(LENGTHS), seed=10 + nh)
    before = _snapshot(b)
    launch(b, lay.desc())
    check_isolation(b, before, _rows(lay))
    check(b, name="lengths")


REGIMES = [(1, ("flat",)), (33, ("flat",)), (129, ("flat",)), (257, ("flat",)), (512, ("flat",)),
           (65, ("sat", 0, 0)), (289, ("sat", 0, 0)),                       # key 0
           (129, ("sat", 128, 0)), (257, ("sat", 256, 0)), (383, ("sat", 382, 0)),   # the last valid key T - 1
           (45, ("sat", 40, 0)), (287, ("sat", 270, 0)),                    # inside the partial last block
           (383, ("sat", 300, 0)),                                          # second 256-key chunk: the first one rescaled
           (511, ("sat", 400, 128)), (300, ("sat", 10, 256)),               # the maximum of the queries of a later pass only
           (100, ("wide",)), (300, ("wide",)),
           (64, ("mean",)), (300, ("mean",)),
           (64, ("range",)), (300, ("range",)), (512, ("range",))]


@pytest.mark.parametrize("nh", HEADS)
@pytest.mark.parametrize("kind", KINDS)
def test_value_regimes_against_fp64(kind, nh):
    """Flat keys, a saturated key at key 0 / T - 1 / inside the partial last block / in the second chunk / for a later query pass
    only, wide scores (fp16 P subnormal and zero), V with a large common mean, K and V at +-65504 -- one launch."""
    lens = [t for t, _ in REGIMES]
    lay = Layout(lens, kind, seed=2)
    b = Bufs(kind, nh, lay)
    fill(b, [sp for _, sp in REGIMES], seed=20 + nh)
    before = _snapshot(b)
    launch(b, lay.desc())
    check_isolation(b, before, _rows(lay))
    check(b, name="regimes")
    for s, (T, sp) in enumerate(REGIMES):  # the regimes are what they claim to be, on the operands the kernel read
        _, _, sc, _ = reference(kind, *operands(b, s))
        if sp[0] == "sat":
            p, q0 = sp[1], sp[2]
            others = torch.cat([sc[:, q0:, :p], sc[:, q0:, p + 1:]], -1).max(-1).values
            assert bool((sc[:, q0:, p] - others >= 30).all()), (T, sp)
            assert q0 == 0 or bool((sc[:, :q0].argmax(-1) != p).all())
        if sp[0] == "wide":
            rel2 = (sc - sc.max(-1, keepdim=True).values) * LOG2E
            assert bool(((rel2 < -14) & (rel2 > -24)).any()) and bool((rel2 < -25).any())


@pytest.mark.parametrize("nh", HEADS)
@pytest.mark.parametrize("kind", (0, 1))
def test_cls_only_rows_equal_the_full_launch(kind, nh):
    """cls_only + q_compact (the encoder's last layer): row s, from the query in row s of the Q columns, equals row tok0 of the full
    launch on the same Q bit for bit, at lengths on both sides of 256; every other ctx row stays the NaN pattern, and the Q columns of
    the rows that are no sequence's row s are NaN.  Kind 0 also without q_compact (query row tok0, output row s)."""
    lens = (1, 33, 128, 200, 255, 256, 257, 300, 383, 512)
    lay = Layout(lens, kind, seed=3)
    b = Bufs(kind, nh, lay)
    fill(b, [("ord",)] * len(lens), seed=30 + nh)
    launch(b, lay.desc())
    check(b, name="cls full")
    full = b.ctx.clone()
    H, n = b.H, len(lens)
    qfull = b.qk.clone()
    b.qk[:, :H] = _nan((lay.rows, H), b.qk.dtype)
    for s in range(n):
        b.qk[s, :H] = qfull[lay.tok0[s], :H]
    modes = ((1,), (0,)) if kind == 0 else ((1,),)
    for (qc,) in modes:
        if not qc:
            b.qk.copy_(qfull)
        b.fresh_ctx()
        before = _snapshot(b)
        launch(b, lay.desc(), cls_only=1, q_compact=qc)
        check_isolation(b, before, list(range(n)))
        for s in range(n):
            assert torch.equal(_bits(b.ctx[s]), _bits(full[lay.tok0[s]])), (qc, s, lens[s])
        check(b, cls=True, compact=bool(qc), name="cls q_compact=%d" % qc)


@pytest.mark.parametrize("nh", HEADS)
@pytest.mark.parametrize("kind", KINDS)
def test_outputs_ignore_batch_mates_order_placement_and_max_len(kind, nh):
    """A sequence's output bits do not depend on its batch mates, the descriptor order (plan_kernel's and a random permutation),
    its tok0 / vcol, or the launch's max_seq_len (128 / 256 / 512: the split kernel's kchunk and every kernel's LDS size)."""
    lay = Layout(LENGTHS, kind, seed=4)
    b = Bufs(kind, nh, lay)
    g = torch.Generator(device="cuda").manual_seed(40 + nh)
    datas = [seq_data(T, nh, ("ord",), g) for T in LENGTHS]
    fill(b, None, 0, datas)
    launch(b, lay.desc())
    ref = b.ctx.clone()

    def same(bb, s, s_ref):
        t, tr, T = bb.lay.tok0[s], lay.tok0[s_ref], LENGTHS[s_ref]
        return torch.equal(_bits(bb.ctx[t:t + T]), _bits(ref[tr:tr + T]))

    if kind != 2:  # the fp32 kernel takes seq_off, in sequence order
        perm = list(np.random.default_rng(5).permutation(len(LENGTHS)))
        b.fresh_ctx()
        launch(b, lay.desc(order=perm))
        assert torch.equal(_bits(b.ctx), _bits(ref)), "descriptor order changed the output"
    # every third sequence, elsewhere in the buffers, without the others
    sub = list(range(0, len(LENGTHS), 3))
    lay2 = Layout([LENGTHS[s] for s in sub], kind, seed=6, first=37)
    b2 = Bufs(kind, nh, lay2)
    fill(b2, None, 0, [datas[s] for s in sub])
    launch(b2, lay2.desc())
    assert lay2.tok0 != [lay.tok0[s] for s in sub]
    for i, s in enumerate(sub):
        assert same(b2, i, s), "sequence %d (T=%d) changed with its batch mates / tok0 / vcol" % (s, LENGTHS[s])
    # the sequences of <= 128 tokens at max_seq_len 128, 256 and 512
    short = [s for s in range(len(LENGTHS)) if LENGTHS[s] <= 128]
    lay3 = Layout([LENGTHS[s] for s in short], kind, seed=7)
    b3 = Bufs(kind, nh, lay3)
    fill(b3, None, 0, [datas[s] for s in short])
    for msl in (128, 256, 512):
        b3.fresh_ctx()
        launch(b3, lay3.desc(), max_seq_len=msl)
        for i, s in enumerate(short):
            assert same(b3, i, s), "max_seq_len %d changed sequence %d (T=%d)" % (msl, s, LENGTHS[s])


@pytest.mark.parametrize("kind", KINDS)
def test_heads_0_to_11_of_16_equal_a_12_head_launch(kind):
    lens = (1, 33, 100, 129, 257, 300, 512)
    g = torch.Generator(device="cuda").manual_seed(50)
    datas = [seq_data(T, 16, ("ord",), g) for T in lens]
    outs = []
    for nh in (16, 12):
        lay = Layout(lens, kind, seed=8)
        b = Bufs(kind, nh, lay)
        fill(b, None, 0, datas)
        launch(b, lay.desc())
        if nh == 16:
            check(b, name="heads")
        outs.append((b, _rows(lay)))
    (b16, rows), (b12, _) = outs
    if kind == 1:  # pair rows: the first 12 heads are the first 768 columns of both halves
        hc16, lc16, _ = _pair_cols(1024)
        hc12, lc12, _ = _pair_cols(768)
        a = torch.cat([b16.ctx[rows][:, hc16[:768]], b16.ctx[rows][:, lc16[:768]]], 1)
        c = torch.cat([b12.ctx[rows][:, hc12], b12.ctx[rows][:, lc12]], 1)
    else:
        a, c = b16.ctx[rows][:, :768], b12.ctx[rows][:, :768]
    assert torch.equal(_bits(a), _bits(c))


@pytest.mark.parametrize("kind", KINDS)
def test_encoder_micro_batch_shape(kind):
    """1,024 sequences x 128 tokens at 12 heads, packed as plan_kernel packs them: a fixed sample of sequences against fp64, every
    output finite, nothing outside them written."""
    n, T = 1024, 128
    lay = Layout([T] * n, kind, seed=9, gaps=False, first=0)
    b = Bufs(kind, 12, lay)
    g = torch.Generator(device="cuda").manual_seed(60)
    H = b.H
    rows = n * T
    if kind == 0:
        b.qk[:rows, :H] = (torch.randn((rows, H), generator=g, device="cuda") * (LOG2E / 8.0)).half()
        b.qk[:rows, H:2 * H] = torch.randn((rows, H), generator=g, device="cuda").half()
        b.vt[:, :rows] = torch.randn((H, rows), generator=g, device="cuda").half()
    else:
        b.qk[:rows] = torch.randn((rows, 3 * H), generator=g, device="cuda")
    before = _snapshot(b)
    launch(b, lay.desc(), max_seq_len=128)
    check_isolation(b, before, list(range(rows)))
    check(b, seqs=(0, 1, 2, 255, 256, 511, 512, 777, 1022, 1023), name="micro-batch")
