"""Rounding-adversarial corpora for the two-precision search (pure NumPy; shared by test_search_adversarial_fixture.py,
which proves on the CPU that a fixture is what it claims to be, and test_gpu_search_adversarial.py, which runs it).

The filter of ance_amd/csrc/search_filter.h may drop a row only when its approximate score s~ (fp16 operands, fp32
accumulation) lies more than 2 eps below the k-th best s~.  On LayerNorm-distributed or clustered rows the fp16 rounding
errors of a score cancel and the real error is ~ eps / sqrt(d): a slack ten times too small goes unnoticed.  Here every
rounding error of a row points the same way:

  tie columns   query 1.0; VICTIMS hold 1 + 2^-11 (an fp16 tie that rounds DOWN to 1.0), IMPOSTORS 1 + 3 * 2^-11 (a tie that
                rounds UP to 1 + 2^-9): exact difference 2^-10 per column, approximate difference 2^-9;
  bump columns  query 1.0; impostors hold 1.0, victims fp16-exact values whose total lift over the impostors is
                B = T * 2^-10 + g (T tie columns, g = 2^-6).  So a victim beats an impostor by exactly g in the exact
                score and LOSES by T * 2^-10 - g in the approximate one: 30-35 % of the kernel's 2 eps (the ceiling of any
                such construction is 2^-10 / (2 * 1.25 * 2^-10) = 40 %);
  rows are made distinct (no duplicate class for the image to collapse) by moving fp16-exact amounts between the two
  columns of a bump pair, which changes no score of the tie query.

The k victims are the exact top-k of the tie query, k' >= k impostors hold the k best approximate scores.  FILLERS are tie
rows with a number of columns negated: same norm (the kernel's eps scales with the maximum norm), scores spread from -d/2
to d/2 in steps of 2.  (Fillers that all score ~0 would sit inside ONE error band: a corpus split that holds only fillers
could then not prune its list, the query would be redone by the exact scan and every GPU test would pass vacuously.)  The
shard is the positive rows plus the exact negation of each, so its mean row is exactly 0; the queries come in +/- pairs,
so the mean query is exactly 0 (or exactly the common component c of the query-mean kind).  All values are small dyadic
numbers: every product and every partial sum is exact in fp32 in ANY order, approximate scores included.
"""
import functools
from types import SimpleNamespace

import numpy as np

G_UNITS = 16          # g = 2^-6 in units of 2^-10
N_BUMP = 8            # four bump pairs, moves of 0..7 units each: 4,096 distinct rows per kind
N_CCOL = 8            # columns that carry the common query component of the query-mean kind
C_VALUE = 2.0         # ... its value there: |mq| = 2 sqrt(8) against 0.05 max|x| ~ 0.05 sqrt(d)
C_ROW = 2.0 ** -4     # what every positive row holds there: bias b = mq . x' = +-1, small against the scores of the tie query / 4
SHIFT = 4.0           # the centred kind: every element shifted by this fp32-exact constant
BAND_MAX = 1536       # rows a query may have within 2 eps of its k-th best approximate score (a list holds 1,792 after a prune)
U10, U11 = 2.0 ** -10, 2.0 ** -11
PLACEMENTS = ("imp_first", "vic_first", "shuffled")


def _moves(i, n_pairs):
    """Digits of i in base 8: units of 2^-10 moved from the second to the first column of every bump pair."""
    out = np.zeros(n_pairs, np.int64)
    for p in range(n_pairs):
        out[p] = i % 8
        i //= 8
    assert i == 0, "more rows of one kind than distinct bump patterns"
    return out


@functools.lru_cache(maxsize=None)
def build(d, n, k, placement, kind="uncentred", seed=0, signs=False, mates=0, nq_tile=0, n_imp=0):
    """kind: 'uncentred' | 'centred' (rows + SHIFT: mu = SHIFT exactly, fl32(x - mu) = the uncentred rows) | 'qmean' (queries
    c + u and c - u: the bias build of the filter).  placement: PLACEMENTS, or 'late' (impostors and victims after all
    fillers: with the default prune schedule no prune sees both groups, the rescore band is the only cut between them).
    signs: query and rows multiplied element-wise by one +-1 vector.  mates: LayerNorm queries (each with its negation)
    as batch mates of the uncentred kind.  nq_tile: repeat the query block up to this many queries (a planner needs
    65,536 / S queries before it keeps S corpus splits).  n_imp: impostors when not k + 8 -- a list's threshold is only
    tight once the list holds k impostors, and shuffled rows spread them over the S corpus splits.  The result is cached:
    treat it as read-only."""
    assert n % 2 == 0 and kind in ("uncentred", "centred", "qmean")
    rng = np.random.default_rng(seed)
    n_c = N_CCOL if kind == "qmean" else 0
    T = d - N_BUMP - n_c                    # tie columns [0, T), bump columns [T, T + N_BUMP), c columns after them
    du = T + N_BUMP                         # columns the tie query lives on
    n_imp = n_imp or min(k + 8, BAND_MAX - k)  # k + 8; k at k = 768, where k + 8 would put 1,544 rows into the band
    n_pos = n // 2
    n_fill = n_pos - k - n_imp
    assert n_imp >= k and n_fill > 0
    n_pairs = N_BUMP // 2

    vic = np.full((k, d), 1.0 + U11)
    lift = T + G_UNITS                      # B in units of 2^-10, spread over the bump columns
    base = np.full(N_BUMP, lift // N_BUMP, np.int64)
    base[0] += lift - base.sum()
    assert base.min() >= 7
    for i in range(k):
        u = base.copy()
        m = _moves(i, n_pairs)
        u[0::2] += m
        u[1::2] -= m
        vic[i, T:du] = 1.0 + u * U10
    imp = np.full((n_imp, d), 1.0 + 3 * U11)
    for i in range(n_imp):
        m = _moves(i, n_pairs)
        imp[i, T:du:2] = 1.0 + m * U10
        imp[i, T + 1:du:2] = 1.0 - m * U10
    fill = np.where(rng.random((n_fill, d)) < 0.5, 1.0 + U11, 1.0 + 3 * U11)
    fill[:, T:du] = 1.0
    n_neg = rng.integers(du // 4, 3 * du // 4 + 1, size=n_fill)
    order = np.argsort(rng.random((n_fill, du)), axis=1)
    neg = order < n_neg[:, None]            # exactly n_neg[i] columns of filler i negated
    fill[:, :du] = np.where(neg, -fill[:, :du], fill[:, :du])
    if n_c:
        vic[:, du:] = imp[:, du:] = fill[:, du:] = C_ROW

    if placement == "imp_first":
        pos, role = np.concatenate([imp, fill, vic]), np.concatenate([np.full(n_imp, 1), np.zeros(n_fill, int), np.full(k, 2)])
    elif placement == "late":
        pos, role = np.concatenate([fill, imp, vic]), np.concatenate([np.zeros(n_fill, int), np.full(n_imp, 1), np.full(k, 2)])
    else:
        pos, role = np.concatenate([vic, fill, imp]), np.concatenate([np.full(k, 2), np.zeros(n_fill, int), np.full(n_imp, 1)])
    x = np.concatenate([pos, -pos])
    role = np.concatenate([role, -role])    # 2 / 1: victim / impostor, -2 / -1: their negations, 0: filler
    if placement == "shuffled":
        perm = rng.permutation(n)
        x, role = x[perm], role[perm]

    u = np.zeros(d)
    u[:du] = 1.0
    q = np.stack([s * 2.0 ** j * u for s in (1.0, -1.0) for j in range(-2, 3)])
    tie_sign = np.array([1] * 5 + [-1] * 5)
    c = np.zeros(d)
    if n_c:
        c[du:] = C_VALUE
        q = q + c[None, :]
    if mates:
        assert kind == "uncentred"
        from oracle import synth
        m = synth.ln_rows(rng, mates, d=d).astype(np.float64)
        q = np.concatenate([q, m, -m])
        tie_sign = np.concatenate([tie_sign, np.zeros(2 * mates, int)])
    if signs:
        s = rng.choice([-1.0, 1.0], size=d)
        x, q, c = x * s, q * s, c * s
    x_unc = x.astype(np.float32)
    assert np.array_equal(x_unc.astype(np.float64), x)
    if kind == "centred":
        x = x + SHIFT
    n_unique = q.shape[0]                   # a tiled query block repeats these rows
    if nq_tile:
        reps = -(-nq_tile // q.shape[0])
        q = np.tile(q, (reps, 1))[:nq_tile]
        tie_sign = np.tile(tie_sign, reps)[:nq_tile]
    x32, q32 = x.astype(np.float32), q.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x) and np.array_equal(q32.astype(np.float64), q)
    for a in (x32, q32, x_unc):
        a.setflags(write=False)
    return SimpleNamespace(x=x32, q=q32, x_unc=x_unc, role=role, tie_sign=tie_sign, n_unique=n_unique, d=d, n=n, k=k, kind=kind, T=T, n_imp=n_imp,
                           mu=np.full(d, SHIFT if kind == "centred" else 0.0, np.float32), mq=c.astype(np.float32),
                           victims=np.flatnonzero(role == 2), neg_victims=np.flatnonzero(role == -2),
                           impostors=np.flatnonzero(role == 1), neg_impostors=np.flatnonzero(role == -1))


# ---- the cases of the GPU file: (d, n, k) x placement x kind -----------------------------------------------------------
SHAPES = [(128, 4096, 1), (128, 16384, 10), (128, 16384, 200), (128, 16384, 768), (768, 8192, 200), (2048, 4096, 50)]
CASES = {}
for _d, _n, _k in SHAPES:
    for _p in PLACEMENTS:
        CASES["unc_d%d_n%d_k%d_%s" % (_d, _n, _k, _p)] = dict(d=_d, n=_n, k=_k, placement=_p, kind="uncentred", mates=16)
for _kind in ("centred", "qmean"):
    for _d, _n, _k in [(128, 16384, 200), (768, 8192, 200)]:
        for _p in PLACEMENTS:
            CASES["%s_d%d_n%d_k%d_%s" % (_kind, _d, _n, _k, _p)] = dict(d=_d, n=_n, k=_k, placement=_p, kind=_kind)
CASES["unc_signs_d128_n16384_k200_shuffled"] = dict(d=128, n=16384, k=200, placement="shuffled", kind="uncentred", signs=True, seed=3)
CASES["qmean_signs_d128_n16384_k200_shuffled"] = dict(d=128, n=16384, k=200, placement="shuffled", kind="qmean", signs=True, seed=4)
# the rescore band as the only cut: 28 rows at the end of the first corpus split, after its last scheduled prune
CASES["noprune_d128_n4096_k10"] = dict(d=128, n=4096, k=10, placement="late", kind="uncentred")
# One knob at a time.  With k = 200 rows shuffled over 8 corpus splits no list holds k impostors and no cut is tight (the
# case checks exactness under the knob, not the slack); the ordered placement puts impostors and victims into different
# splits (the victims meet the threshold their sibling published), the 4,096-row shard puts them into the same lists.
KNOB_CASES = ["unc_d128_n16384_k200_shuffled", "unc_d128_n16384_k200_imp_first", "unc_d128_n4096_k1_shuffled"]
# ANCE_FAST_SPLITS is only a lower bound while a launch has fewer than 256 workgroups: 65,536 / S queries pin S.  Besides
# the shuffled k = 200 rows: the ordered placements (windows of 8 tiles: impostors in the first tile of split 0, victims
# in the last tile of split S - 1, or the other way round: what crosses between the splits decides) and k = 10 with 24 k
# impostors, shuffled (every list holds more than k impostors AND a victim or two).
SPLIT_VARIANTS = {"k200_shuffled": dict(k=200, placement="shuffled"), "k200_imp_first": dict(k=200, placement="imp_first"),
                  "k200_vic_first": dict(k=200, placement="vic_first"), "k10_dense_shuffled": dict(k=10, placement="shuffled", n_imp=240)}
SPLIT_CASES = {(s, w, v): dict(d=128, n=16384, kind="uncentred", mates=16, nq_tile=65536 // s, **kw)
               for s, w in [(2, 0), (2, 8), (4, 8), (8, 8)] for v, kw in SPLIT_VARIANTS.items()}


def fixture(name):
    return build(**CASES[name])


# ---- what the device does with a fixture, restated ------------------------------------------------------------------------
def colsum_mean(a):
    """(mean, partials exact?) as idx_colsum_kernel + idx_mean_kernel compute it: fp32 partial b sums the rows b, b + n_part, ...
    in that order, n_part = min(ceil(n / 1024), 1024); then a double sum over the partials, divided by n, rounded to fp32."""
    n, d = a.shape
    n_part = min(-(-n // 1024), 1024)
    steps = -(-n // n_part)
    pad = np.zeros((steps * n_part, d), np.float32)
    pad[:n] = a
    pad = pad.reshape(steps, n_part, d)
    acc = np.zeros((n_part, d), np.float32)
    for s in range(steps):
        acc = (acc + pad[s]).astype(np.float32)
    exact = np.array_equal(acc.astype(np.float64), pad.astype(np.float64).sum(axis=0))
    return (acc.astype(np.float64).sum(axis=0) / n).astype(np.float32), exact


def query_mean(q):
    """The mean query of a call: ip_topk_fast runs the same two kernels over the queries with min(nq, 1024) partials."""
    nq, d = q.shape
    n_part = min(nq, 1024)
    acc = np.zeros((n_part, d), np.float32)
    for s in range(-(-nq // n_part)):
        blk = q[s * n_part:(s + 1) * n_part]
        acc[:len(blk)] = (acc[:len(blk)] + blk).astype(np.float32)
    return (acc.astype(np.float64).sum(axis=0) / nq).astype(np.float32)


def plan_splits(n, nq, k, knob=0):
    """Corpus splits make_fast_plan (ip_topk_fast.hip) picks."""
    n_tiles, nqt = -(-n // 256), -(-nq // 256)
    S = knob
    if S < 1 or S > 32 or S & (S - 1):
        S = 2
    while nqt * S < 256 and S < 32:
        S *= 2
    p2 = lambda v: 1 << max(v - 1, 0).bit_length()
    while S > 1 and (S * 8 > n_tiles or p2((S + 4) * k) > 8192):
        S //= 2
    return S


def scheduled_prunes(k, tiles, prune_at=512, growth=150):
    """Tile counts (1-based, per split) after which ip_topk_fast_kernel prunes every list on schedule."""
    at = min(max(prune_at, k + 64), 2048 - 256)
    nxt, out = max(1, -(-at // 256)), []
    while nxt <= tiles:
        out.append(nxt)
        nxt = max(nxt + 1, nxt * growth // 100)
    return out
