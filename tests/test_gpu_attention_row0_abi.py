"""The first-row attention core at its C ABI (include/ance_amd.h: ance_attention_row0_*; csrc/attention_row0.hip), called directly on
caller-owned, sentinel-filled buffers: the padded form, seq_rows below max_seq_len, the packed form, hostile descriptors, strides
wider than 64 n_heads on all eight matrices, the workspace's extent, a host (seed, offset) with a non-zero high word, and the copy
path of ance_amd.attention.attention_first_row.

Numbers: model_util.check -- attention_train_util.bound for fp32, attention_half_util.bound16 for 16 bits -- against
model_util.first_row_fp64 at the lengths the header's clamps leave, with the eager expression's own distance; every measured
distance is printed.  Everything "untouched" is exact equality with the sentinel, a NaN with a recognisable payload; everything
"zero" is exactly +0.0.

Guards: every buffer is sized so that a kernel WITHOUT its clamps would still stay inside the allocation (_geometry_is_safe): a
defect shows as a failed sentinel assertion, never as a fault."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import attention_train_util as A
import model_util as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 0x5EED0123456789AB
NAN32 = 0x7FC00ABC   # tests/test_gpu_attention_train.py's sentinel
# dtype name -> (torch dtype, the integer type of its bits, the sentinel, model_util's dtype argument)
TYPES = {"fp32": (torch.float32, torch.int32, NAN32, None),
         "fp16": (torch.float16, torch.int16, 0x7DAB, torch.float16),     # tests/test_gpu_attention_half.py's
         "bf16": (torch.bfloat16, torch.int16, 0x7FCB, torch.bfloat16)}
PAD_COLS, Q_GUARD, WS_GUARD = 8, 4, 64
OUTPUTS, INPUTS = ("ctx", "dq", "dk", "dv"), ("q", "k", "v", "dctx")

_reference = functools.lru_cache(maxsize=None)(M.reference)


def _code(dt):
    from ance_amd import _lib
    return dict(fp32=_lib.ANCE_DTYPE_F32, fp16=_lib.ANCE_DTYPE_F16, bf16=_lib.ANCE_DTYPE_BF16)[dt]


class Buf:
    """rows x (H + PAD_COLS) elements between `lead` and `trail` guard rows, everything the sentinel; x (np, NaN allowed) goes into
    the first H columns of the rows in between.  ptr: the address of row 0."""

    def __init__(self, dt, rows, H, lead, trail, x=None):
        self.io, it, self.sent, _ = TYPES[dt]
        self.rows, self.H, self.lead = rows, H, lead
        self.t = torch.full((lead + rows + trail, H + PAD_COLS), self.sent, dtype=it, device=DEV)
        if x is not None:
            self.t.view(self.io)[lead:lead + rows, :H] = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV).to(self.io)
        self.ptr = self.t[lead:].data_ptr()
        assert self.ptr % 16 == 0
        self.before = self.bits()

    def bits(self):
        return self.t.cpu().numpy().copy()

    def values(self):
        """fp32 values of the rows between the guards, first H columns."""
        return self.t.view(self.io)[self.lead:self.lead + self.rows, :self.H].float().cpu().numpy()


class Case:
    """One call's geometry and data.  descs: (first, len) per descriptor as the device gets them; the data of a descriptor whose
    clamped length e is positive lies at K/V rows first .. first + e - 1, every other K/V row is NaN, and so are the q and dctx rows
    of descriptors that run nothing."""

    def __init__(self, dt, nh, tag, descs, max_seq_len, seq_rows, n_rows, kv_rows, p=0.0, seed=0, offset=0):
        self.dt, self.nh, self.H, self.tag = dt, nh, 64 * nh, tag
        self.first = np.array([f for f, _ in descs], np.int32)
        self.lens = np.array([n for _, n in descs], np.int32)
        self.max_seq_len, self.seq_rows, self.n_rows, self.kv_rows = max_seq_len, seq_rows, n_rows, kv_rows
        self.p, self.seed, self.offset = p, seed, offset
        # the header's clamps, restated: e = the rows a descriptor attends to, own = the dk / dv rows it owns in the padded form
        self.eff, self.own = [], []
        for f, n in descs:
            inside = 0 <= f < n_rows
            self.eff.append(min(n, max_seq_len, n_rows - f) if inside and n > 0 else 0)
            self.own.append(min(seq_rows, n_rows - f) if inside and seq_rows > 0 else 0)
        self.lead = max([0] + [-f for f, _ in descs]) + max(n for _, n in descs) + 8
        self.trail = max(max(n for _, n in descs), seq_rows) + 8
        self._geometry_is_safe(descs)
        mdt = TYPES[dt][3]
        (q0, k, v, g, _), self.want, self.ref, _ = _reference(tag, tuple(self.eff), nh, max(max(self.eff), 1), 1.0, p, seed, offset, mdt)
        nan = np.float32("nan")
        runs = np.array(self.eff) > 0
        self.q0, self.g = np.where(runs[:, None], q0, nan), np.where(runs[:, None], g, nan)
        self.k, self.v = (np.full((kv_rows, self.H), nan, np.float32) for _ in range(2))
        for s, (f, e) in enumerate(zip(self.first, self.eff)):
            self.k[f:f + e], self.v[f:f + e] = k[s, :e], v[s, :e]

    def _geometry_is_safe(self, descs):
        """The hard rule: a length at most 512 (the kernel's LDS array), and every row a kernel WITHOUT clamps could reach --
        first .. first + max(len, seq_rows) - 1 -- inside the allocation of every K/V-shaped buffer."""
        total = self.lead + self.kv_rows + self.trail
        assert 1 <= self.n_rows <= self.kv_rows
        for f, n in descs:
            assert n <= 512 and self.lead + f >= 0 and self.lead + f + max(n, self.seq_rows, 0) <= total, (f, n)
        covered = np.zeros(self.kv_rows, int)
        for f, e, o in zip(self.first, self.eff, self.own):
            covered[f:f + max(e, o)] += 1
        assert covered.max() <= 1, "two descriptors share K/V rows"

    @property
    def n_seq(self):
        return len(self.first)


class Result:
    pass


def _run(c, n_seq=None, offset=None):
    """Forward and backward through the plain entry points on fresh buffers; everything read back."""
    from ance_amd import _lib
    L = _lib.lib()
    n_seq = n_seq or c.n_seq
    kv = lambda x=None: Buf(c.dt, c.kv_rows, c.H, c.lead, c.trail, x)     # noqa: E731
    qs = lambda x=None: Buf(c.dt, c.n_seq, c.H, Q_GUARD, Q_GUARD, x)      # noqa: E731
    r = Result()
    r.buf = dict(q=qs(c.q0), k=kv(c.k), v=kv(c.v), dctx=qs(c.g), ctx=qs(), dq=qs(), dk=kv(), dv=kv())
    ws_bytes = L.ance_attention_row0_workspace_bytes(n_seq, c.nh)
    assert ws_bytes == (8 * n_seq * c.nh + 255) // 256 * 256
    ws = torch.full((ws_bytes // 4 + 2 * WS_GUARD,), NAN32, dtype=torch.int32, device=DEV)
    first, lens = torch.from_numpy(c.first).to(DEV), torch.from_numpy(c.lens).to(DEV)
    b, ld = r.buf, c.H + PAD_COLS
    a = _lib.AnceAttn16Args(q=b["q"].ptr, k=b["k"].ptr, v=b["v"].ptr, ctx=b["ctx"].ptr, ld_q=ld, ld_k=ld, ld_v=ld, ld_ctx=ld,
                            d_seq_first=first.data_ptr(), d_seq_len=lens.data_ptr(), n_seq=n_seq, max_seq_len=c.max_seq_len,
                            n_rows=c.n_rows, n_heads=c.nh, seq_rows=c.seq_rows, dtype=_code(c.dt), dropout_p=c.p,
                            training=1, seed=c.seed, offset=c.offset if offset is None else offset,
                            d_workspace=ws[WS_GUARD:].data_ptr(), workspace_bytes=ws_bytes)
    gr = _lib.AnceAttn16GradArgs(dctx=b["dctx"].ptr, dq=b["dq"].ptr, dk=b["dk"].ptr, dv=b["dv"].ptr, ld_dctx=ld, ld_dq=ld, ld_dk=ld,
                                 ld_dv=ld)
    st = _lib.current_stream_ptr()
    _lib.check(L.ance_attention_row0_forward(ctypes.byref(a), st), "ance_attention_row0_forward")
    _lib.check(L.ance_attention_row0_backward(ctypes.byref(a), ctypes.byref(gr), st), "ance_attention_row0_backward")
    torch.cuda.synchronize()
    r.n_seq, r.ws_bits, r.ws = n_seq, ws.cpu().numpy(), ws.view(torch.float32).cpu().numpy()
    r.bits = {n: x.bits() for n, x in b.items()}
    r.values = {n: b[n].values() for n in OUTPUTS}
    return r


def _check_footprint(c, r):
    """Every byte of the four outputs and of the workspace is either the sentinel or what the contract says is written there."""
    n_seq, H = r.n_seq, c.H
    for n in INPUTS:
        assert np.array_equal(r.bits[n], r.buf[n].before), n + " has changed"
    sent = r.buf["ctx"].sent
    for n in ("ctx", "dq"):                                     # [n_seq, H]: row s, zeros when the descriptor runs nothing
        bits, val = r.bits[n], r.values[n]
        assert np.all(bits[:Q_GUARD] == sent) and np.all(bits[Q_GUARD + n_seq:] == sent), n + ": guard rows, rows >= n_seq"
        assert np.all(bits[:, H:] == sent), n + ": columns past 64 n_heads"
        for s in range(n_seq):
            if c.eff[s] == 0:
                assert np.all(bits[Q_GUARD + s, :H] == 0), (n, s, "a descriptor that runs nothing leaves exact zeros")
            else:
                assert np.all(np.isfinite(val[s])), (n, s)
    for n in ("dk", "dv"):
        bits, val = r.bits[n], r.values[n]
        kind = np.zeros(bits.shape, np.int8)                    # 0: untouched, 1: a valid row, 2: a pad row of the padded form
        for s in range(n_seq):
            f, e, o = c.lead + int(c.first[s]), c.eff[s], c.own[s]
            kind[f:f + e, :H] = 1
            kind[f + e:f + o, :H] = 2
        assert np.all(bits[:c.lead] == sent) and np.all(bits[c.lead + c.kv_rows:] == sent), n + ": guard rows"
        assert np.all(bits[c.lead + c.n_rows:] == sent), n + ": rows at and behind n_rows"
        assert np.all(bits[:, H:] == sent), n + ": columns past 64 n_heads"
        assert np.all(bits[kind == 0] == sent), n + ": rows that no sequence covers (or owns)"
        assert np.all(bits[kind == 2] == 0), n + ": the pad rows of the padded form are exactly +0.0"
        assert np.all(np.isfinite(val[kind[c.lead:c.lead + c.kv_rows, :H] == 1])), n
    # the workspace: (m, l) of the sequences that ran, and nothing else
    written = np.zeros(r.ws_bits.shape, bool)
    for s in range(n_seq):
        if c.eff[s] > 0:
            written[WS_GUARD + 2 * s * c.nh:WS_GUARD + 2 * (s + 1) * c.nh] = True
    assert np.all(r.ws_bits[~written] == NAN32), "workspace: guards, skipped sequences and the tail stay"
    ml = r.ws[written].reshape(-1, 2)
    assert np.all(np.isfinite(ml)) and np.all(ml[:, 1] >= 1.0), "workspace: (max, sum >= 1) of every (sequence, head) that ran"


def _got(c, r, n_seq=None):
    """The outputs in model_util's shapes: ctx, dq [B, H]; dk, dv [B, L, H] with the valid rows of every sequence, zeros elsewhere."""
    B, Lr = c.n_seq, c.want["dk"].shape[1]
    got = dict(ctx=np.zeros((B, c.H), np.float32), dq=np.zeros((B, c.H), np.float32), dk=np.zeros((B, Lr, c.H), np.float32),
               dv=np.zeros((B, Lr, c.H), np.float32))
    for s in range(n_seq or r.n_seq):
        f, e = int(c.first[s]), c.eff[s]
        if e > 0:
            got["ctx"][s], got["dq"][s] = r.values["ctx"][s], r.values["dq"][s]
            got["dk"][s, :e], got["dv"][s, :e] = r.values["dk"][f:f + e], r.values["dv"][f:f + e]
    return got


# ---------------------------------------------------------------------------------------------------------------- a. the three forms
def _form(form, dt, nh):
    if form == "padded":        # seq_rows = max_seq_len = L
        lens, L = (96, 31, 0, 7), 96
        return Case(dt, nh, "abi.padded", [(s * L, n) for s, n in enumerate(lens)], L, L, len(lens) * L, len(lens) * L)
    if form in ("narrow", "narrow_gap"):   # seq_rows 40 below max_seq_len 64; narrow_gap: 8 rows nobody owns between the sequences
        lens, pitch = (40, 39, 1, 0, 17), 40 if form == "narrow" else 48
        return Case(dt, nh, "abi.narrow", [(s * pitch, n) for s, n in enumerate(lens)], 64, 40, len(lens) * pitch, len(lens) * pitch)
    lens, L = (33, 5, 0, 96, 1), 96   # packed: attention_train_util.pack's rows, d_seq_first the cumulative offsets
    off = A.pack(np.zeros((len(lens), L, 1), np.float32), np.array(lens))[1]
    return Case(dt, nh, "abi.packed", [(int(off[s]), n) for s, n in enumerate(lens)], L, 0, int(off[-1]), int(off[-1]))


FORM_CASES = [(dt, 12, form) for form in ("padded", "narrow", "narrow_gap", "packed") for dt in ("fp32", "fp16", "bf16")] \
    + [("bf16", 16, "packed")]


@pytest.mark.parametrize("dt,nh,form", FORM_CASES, ids=["%s-%d-%s" % c for c in FORM_CASES])
def test_guarded_buffers_in_the_three_forms(dt, nh, form):
    """Stride 64 n_heads + 8 on all eight matrices.  Guard rows and the stride's unused columns of ctx, dq, dk, dv keep the sentinel;
    padded / narrow: rows len .. seq_rows - 1 of every sequence in dk, dv are exactly +0.0 and rows nobody owns keep the sentinel;
    packed: every row no sequence covers keeps it; a sequence of length 0 has exact-zero ctx[s], dq[s]; q, k, v, dctx keep their
    bits; of the NaN-filled workspace only (m, l) of the sequences that ran is written, so the backward reads nothing of a skipped
    one; everything defined is finite with NaN in every K / V row outside a sequence; the values meet model_util.check."""
    c = _form(form, dt, nh)
    r = _run(c)
    _check_footprint(c, r)
    got = _got(c, r)
    if form == "packed":   # the same through attention_train_util.unpack of the packed rows
        ln = np.array(c.eff)
        for n in ("dk", "dv"):
            assert np.array_equal(got[n], A.unpack(r.values[n][:c.n_rows], ln, c.max_seq_len)), n
    M.check("C ABI %s %s %d heads, stride %d" % (form, dt, nh, c.H + PAD_COLS), got, c.want, c.ref, TYPES[dt][3])


# ---------------------------------------------------------------------------------------------------------------- b. hostile descriptors
HOSTILE_L = 64


def _hostile(form, dt, tail_len):
    """Two well-formed descriptors, then: a length above max_seq_len (200 -> 64); a length (tail_len) that, from its first row, ends
    past -- or, tail_len = 10, inside -- an n_rows that ends 30 rows behind that first row, inside the buffer; a negative length; first
    = -3; first = n_rows + 2 (inside the trailing rows of the buffer)."""
    L = HOSTILE_L
    if form == "padded":
        # rows 192 .. 255 belong to the negative length: a sequence of length <= 0 in the padded form has all its rows zeroed
        n_rows = 256 + 30
        descs = [(0, 20), (L, L), (2 * L, 200), (4 * L, tail_len), (3 * L, -5), (-3, 20), (n_rows + 2, 20)]
        return Case(dt, 12, "abi.hostile", descs, L, L, n_rows, 5 * L)
    n_rows = 148 + 30
    descs = [(0, 20), (20, L), (84, 200), (148, tail_len), (148, -5), (-3, 20), (n_rows + 2, 20)]
    return Case(dt, 12, "abi.hostile", descs, L, 0, n_rows, 148 + L)


@pytest.mark.parametrize("form,tail_len", [("padded", 50), ("padded", 10), ("packed", 50)])
@pytest.mark.parametrize("dt", ["fp32", "fp16"])
def test_hostile_descriptors(dt, form, tail_len):
    """No row >= n_rows is touched whatever the descriptors say.  The clamped lengths give the fp64 statement at the clamped
    length; nothing at or behind row n_rows is written, and in the padded form the zeroed rows stop there too (tail_len = 10: rows
    10 .. 29 of that sequence are zeros, rows 30 .. 63 keep the sentinel).  A negative length, first = -3 and first = n_rows + 2 leave
    exact zeros in ctx[s] and dq[s]; the two whose first row is outside [0, n_rows) touch nothing in dk and dv in either form, the
    negative length nothing in the packed form and -- a sequence of length <= 0 -- zeros in the rows it owns in the padded form.
    The well-formed sequences' results are the bits of a call without the hostile descriptors."""
    c = _hostile(form, dt, tail_len)
    assert c.eff == [20, 64, 64, min(tail_len, 30), 0, 0, 0]
    assert c.own == ([64, 64, 64, 30, 64, 0, 0] if form == "padded" else [0] * 7)
    r = _run(c)
    _check_footprint(c, r)
    for n in ("dk", "dv"):     # said again by row number: the hostile first rows' neighbourhoods, and n_rows onwards
        bits, sent = r.bits[n], r.buf[n].sent
        assert np.all(bits[c.lead - 3 - 64:c.lead] == sent) and np.all(bits[c.lead + c.n_rows:] == sent), n
    M.check("C ABI hostile %s %s tail %d" % (form, dt, tail_len), _got(c, r), c.want, c.ref, TYPES[dt][3])
    plain = _run(c, n_seq=2)
    _check_footprint(c, plain)
    for n in OUTPUTS:
        a, b = _got(c, r, 2)[n], _got(c, plain, 2)[n]
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), n + ": the well-formed sequences, with and without the hostile ones"


# ---------------------------------------------------------------------------------------------------------------- c. the host pair's high words
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_host_offset_with_a_high_word(dt):
    """dropout_p = 0.5 under (seed, offset) = (0x5EED0123456789AB, 2^32 + 5) through the plain calls, against the mask restated by
    model_util.first_row_keep at that pair; the masks at offset 5 differ, so the bits do."""
    lens, L = (1, 5, 64, 96, 0), 96
    descs = [(s * L, n) for s, n in enumerate(lens)]
    c = Case(dt, 12, "abi.offset", descs, L, L, len(lens) * L, len(lens) * L, 0.5, SEED, 2 ** 32 + 5)
    r = _run(c)
    _check_footprint(c, r)
    M.check("C ABI p=0.5 offset 2^32 + 5 %s" % dt, _got(c, r), c.want, c.ref, TYPES[dt][3])
    keep_hi = M.first_row_keep(0.5, SEED, 2 ** 32 + 5, lens, 12, L)
    keep_lo = M.first_row_keep(0.5, SEED, 5, lens, 12, L)
    assert not np.array_equal(keep_hi[3, :, :96], keep_lo[3, :, :96])
    low = _run(c, offset=5)
    for n in OUTPUTS:
        assert not np.array_equal(r.bits[n], low.bits[n]), n + ": the high word of the offset does not reach the kernel"
    c_lo = Case(dt, 12, "abi.offset", descs, L, L, len(lens) * L, len(lens) * L, 0.5, SEED, 5)
    M.check("C ABI p=0.5 offset 5 %s" % dt, _got(c_lo, low), c_lo.want, c_lo.ref, TYPES[dt][3])


# ---------------------------------------------------------------------------------------------------------------- d. the wrapper's copy path
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_the_wrapper_copies_views_it_cannot_pass(dt):
    """k, v as columns 2 .. 2 + H of a wider buffer (a base that is not 16-byte aligned) and q0 with a row stride of H + 2 (no multiple
    of a piece): _rows copies all three, and the output and the three gradients arrive in the views' own positions with the bits of
    the contiguous call."""
    from ance_amd.attention import _rows, attention_first_row
    io, _, _, mdt = TYPES[dt]
    piece, prec = (4, "fp32") if dt == "fp32" else (8, "half")
    lens, L, H = (96, 31, 0, 7), 96, 768
    (q0, k, v, g, ln), want, ref, _ = _reference("abi.padded", lens, 12, L, 1.0, 0.0, 0, 0, mdt)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV).to(io)   # noqa: E731
    tl, tg = torch.from_numpy(ln).to(DEV), dev(g)

    tq, tk, tv = (dev(x).requires_grad_(True) for x in (q0, k, v))
    ctx = attention_first_row(tq, tk, tv, tl, 12, precision=prec)
    ctx.backward(tg)
    plain = dict(ctx=ctx.detach(), dq=tq.grad, dk=tk.grad, dv=tv.grad)
    M.check("wrapper, contiguous %s" % dt, {n: t.float().cpu().numpy() for n, t in plain.items()}, want, ref, mdt)

    wq = torch.zeros(len(lens), H + 2, dtype=io, device=DEV)
    wk, wv = (torch.zeros(len(lens), L, H + 8, dtype=io, device=DEV) for _ in range(2))
    wq[:, :H], wk[..., 2:2 + H], wv[..., 2:2 + H] = dev(q0), dev(k), dev(v)
    for w in (wq, wk, wv):
        w.requires_grad_(True)
    vq, vk, vv = wq[:, :H], wk[..., 2:2 + H], wv[..., 2:2 + H]
    assert vk.data_ptr() % 16 and vv.data_ptr() % 16 and vq.stride(0) % piece
    for t in (vq, vk, vv):
        assert _rows(t, piece)[0].data_ptr() != t.data_ptr(), "a view the kernels cannot read is copied"
    out = attention_first_row(vq, vk, vv, tl, 12, precision=prec)
    out.backward(tg)
    bits = lambda t: t.contiguous().view(torch.int32 if dt == "fp32" else torch.int16)   # noqa: E731
    assert torch.equal(bits(out.detach()), bits(plain["ctx"]))
    assert torch.equal(bits(wq.grad[:, :H]), bits(plain["dq"])) and not bits(wq.grad[:, H:]).any()
    for w, n in ((wk, "dk"), (wv, "dv")):
        assert torch.equal(bits(w.grad[..., 2:2 + H]), bits(plain[n])), n
        assert not bits(w.grad[..., :2]).any() and not bits(w.grad[..., 2 + H:]).any(), n + ": columns outside the view"
