"""The two-pass softmax of attention_split_kernel (csrc/attention.hip: split_attend_two_pass) -- the form every sequence of <= 128
tokens takes: all scores first, the maximum, then the exponentials, nothing rescaled -- through kind 1 of ance_debug_attention, with
the layout, the fp64 reference and the kind-1 bound of test_gpu_attention.py (that bound is derived for the online form; the two-pass
form does fewer roundings -- no alpha products on the accumulators or on l -- so it holds unchanged).

  1. every length around the 32-key blocks x every value regime against fp64, one launch;
  2. ANCE_ATTN_TWO_PASS=0 (the online form everywhere) against 1: bit-identical where both forms must agree (one key block: the
     online alpha is exp2(-inf) = 0 on zero accumulators; T > 128: not two-pass), within twice the fp64 bound elsewhere (both forms
     lie within the bound of the same reference);
  3. the identities the encoder relies on, bit for bit, on the new form: max_seq_len 128 / 256 / 512, descriptor order, batch mates,
     two runs, cls_only with the compact Q row = row tok0 of the full launch.

12 heads, one launch per case, NaN-patterned gaps and guard rows.  Needs an MI355X."""
import os

import numpy as np
import pytest
import torch

from test_gpu_attention import (Bufs, Layout, _bits, _nan, _rows, _snapshot, check, check_isolation, fill, launch, operands, output,
                                reference, seq_data)

pytestmark = pytest.mark.gpu

NH = 12
KNOB = "ANCE_ATTN_TWO_PASS"
LENGTHS = (1, 31, 32, 33, 64, 65, 96, 97, 127, 128)


def _set_knob(value):
    from ance_amd import _lib
    if value is None:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = value
    _lib.reload_env()


@pytest.fixture(autouse=True)
def two_pass_on():
    """Every test starts on the two-pass form (the default, whatever the environment says) and leaves the knob as it found it."""
    before = os.environ.get(KNOB)
    _set_knob("1")
    try:
        yield
    finally:
        _set_knob(before)


def pm60_data(T, nh, g):
    """Scores near +60 and -60 in natural units (the log2 domain: +-87): half of the keys on each side, in random order -- a softmax
    saturated on the +60 keys, the others 2^-173 of them (exp2 flushes to zero)."""
    rn = lambda *sh: torch.randn(sh, generator=g, device="cuda", dtype=torch.float64)  # noqa: E731
    u = rn(nh, 64)
    u = u / u.norm(dim=-1, keepdim=True)
    orth = lambda x: x - (x * u).sum(-1, keepdim=True) * u  # noqa: E731
    sign = torch.ones((T, 1, 1), device="cuda", dtype=torch.float64)
    sign[torch.randperm(T, generator=g, device="cuda")[: T // 2]] = -1.0
    q = orth(0.3 * rn(T, nh, 64)) + 4.0 * u          # q . k / 8 = +-60 + N(0, ~0.3)
    k = orth(0.5 * rn(T, nh, 64)) + 120.0 * sign * u
    return q, k, rn(T, nh, 64)


def regimes_of(T):
    """The value regimes of test 1 at length T: N(0, 1); one dominant key in the first, a middle and the last key block (the maximum is
    found early or late); all scores equal; scores near +-60."""
    nkb = (T + 31) // 32
    dominant = sorted({min(5, T - 1), min(32 * (nkb // 2) + 7, T - 1), T - 1})
    return [("ord",)] + [("sat", p, 0) for p in dominant] + [("flat",), ("pm60",)]


def data_of(T, spec, g):
    return pm60_data(T, NH, g) if spec[0] == "pm60" else seq_data(T, NH, spec, g)


def test_lengths_and_regimes_against_fp64():
    cases = [(T, sp) for T in LENGTHS for sp in regimes_of(T)]
    lay = Layout([T for T, _ in cases], 1, seed=11)
    b = Bufs(1, NH, lay)
    g = torch.Generator(device="cuda").manual_seed(110)
    fill(b, None, 0, [data_of(T, sp, g) for T, sp in cases])
    before = _snapshot(b)
    launch(b, lay.desc(), max_seq_len=128)
    check_isolation(b, before, _rows(lay))
    check(b, name="two-pass")
    for s, (T, sp) in enumerate(cases):  # the regimes are what they claim to be, on the operands the kernel read
        _, _, sc, _ = reference(1, *operands(b, s))
        if sp[0] == "sat" and T > 1:
            p = sp[1]
            others = torch.cat([sc[:, :, :p], sc[:, :, p + 1:]], -1).max(-1).values
            assert bool((sc[:, :, p] - others >= 30).all()), (T, sp)
        if sp[0] == "flat":
            assert bool(((sc.max(-1).values - sc.min(-1).values) <= 1e-4).all()), (T, sp)
        if sp[0] == "pm60":
            assert bool(((sc.abs() - 60.0).abs() < 5.0).all()), (T, sp)
            assert T == 1 or (bool((sc > 0).any()) and bool((sc < 0).any())), (T, sp)


def test_online_form_against_two_pass_form():
    same = (1, 2, 17, 31, 32, 129, 256, 257)       # one key block, or no two-pass form: the same bits
    close = (33, 64, 65, 96, 97, 127, 128)          # 2 .. 4 key blocks: rounding only
    lens = same + close
    lay = Layout(lens, 1, seed=12)
    b = Bufs(1, NH, lay)
    fill(b, [("ord",)] * len(lens), seed=120)
    outs = {}
    for knob in ("0", "1"):
        _set_knob(knob)
        b.fresh_ctx()
        before = _snapshot(b)
        launch(b, lay.desc(), max_seq_len=512)
        check_isolation(b, before, _rows(lay))
        check(b, name="knob " + knob)
        outs[knob] = b.ctx.clone()
    differing = 0
    for s, T in enumerate(lens):
        rows = slice(lay.tok0[s], lay.tok0[s] + T)
        if T in same:
            assert torch.equal(_bits(outs["0"][rows]), _bits(outs["1"][rows])), "T=%d: the two forms differ" % T
            continue
        _, tol, _, _ = reference(1, *operands(b, s))
        b.ctx = outs["0"]
        o0 = output(b, rows)
        b.ctx = outs["1"]
        o1 = output(b, rows)
        d = (o0 - o1).abs()
        frac = float((d / (2 * tol)).max())
        print("T=%d: max |online - two-pass| = %.3g, %.3g of twice the fp64 bound" % (T, float(d.max()), frac))
        assert bool((d <= 2 * tol).all()), "T=%d: %.3g of twice the bound" % (T, frac)
        differing += int((d > 0).sum())
    assert differing > 0, "ANCE_ATTN_TWO_PASS selects nothing: the forms agree bit for bit at 2 .. 4 key blocks"


def test_two_pass_identities_bit_for_bit():
    lens = (1, 31, 32, 33, 64, 65, 74, 96, 97, 127, 128)
    g = torch.Generator(device="cuda").manual_seed(130)
    datas = [seq_data(T, NH, ("ord",), g) for T in lens]
    lay = Layout(lens, 1, seed=13)
    b = Bufs(1, NH, lay)
    fill(b, None, 0, datas)
    launch(b, lay.desc(), max_seq_len=128)
    check(b, name="identities")
    ref = b.ctx.clone()
    # max_seq_len (the launch's kchunk and LDS size), twice each
    for msl in (128, 256, 512, 128):
        b.fresh_ctx()
        launch(b, lay.desc(), max_seq_len=msl)
        assert torch.equal(_bits(b.ctx), _bits(ref)), "max_seq_len %d (or a second run) changed the output" % msl
    # another descriptor order
    perm = list(np.random.default_rng(14).permutation(len(lens)))
    b.fresh_ctx()
    launch(b, lay.desc(order=perm), max_seq_len=128)
    assert torch.equal(_bits(b.ctx), _bits(ref)), "descriptor order changed the output"
    # other batch mates (online single-chunk and chunked ones among them), other token rows
    sub = list(range(0, len(lens), 2))
    mates = (300, 129, 256)
    lens2 = [lens[s] for s in sub] + list(mates)
    lay2 = Layout(lens2, 1, seed=15, first=41)
    b2 = Bufs(1, NH, lay2)
    fill(b2, None, 0, [datas[s] for s in sub] + [seq_data(T, NH, ("ord",), g) for T in mates])
    launch(b2, lay2.desc(), max_seq_len=512)
    assert lay2.tok0[:len(sub)] != [lay.tok0[s] for s in sub]
    for i, s in enumerate(sub):
        t, tr, T = lay2.tok0[i], lay.tok0[s], lens[s]
        assert torch.equal(_bits(b2.ctx[t:t + T]), _bits(ref[tr:tr + T])), "T=%d changed with its batch mates / tok0" % T


def test_two_pass_cls_only_equals_row_tok0_of_the_full_launch():
    lens = (1, 33, 74, 128)
    lay = Layout(lens, 1, seed=16)
    b = Bufs(1, NH, lay)
    fill(b, [("ord",)] * len(lens), seed=160)
    launch(b, lay.desc(), max_seq_len=128)
    full = b.ctx.clone()
    H, n = b.H, len(lens)
    qfull = b.qk.clone()
    b.qk[:, :H] = _nan((lay.rows, H), b.qk.dtype)  # only the compact rows hold a query
    for s in range(n):
        b.qk[s, :H] = qfull[lay.tok0[s], :H]
    for msl in (128, 512):
        b.fresh_ctx()
        before = _snapshot(b)
        launch(b, lay.desc(), max_seq_len=msl, cls_only=1, q_compact=1)
        check_isolation(b, before, list(range(n)))
        for s in range(n):
            assert torch.equal(_bits(b.ctx[s]), _bits(full[lay.tok0[s]])), (msl, s, lens[s])
    check(b, cls=True, compact=True, name="two-pass cls")
