"""CPU proof that the rounding-adversarial corpora of search_adversarial_util.py are what they claim to be, for every
fixture and shape tests/test_gpu_search_adversarial.py runs: the device's means come out exactly as intended, the mean-query
decision falls on the intended side, the victims are the oracle's top-k, the fp16 filter under-estimates them against their
competitors by >= 28 % of the kernel's own 2 eps, and so few rows lie within 2 eps of the k-th best approximate score that the
fast path -- not the exact-scan redo, which ignores eps -- has to answer.  Run with -s for the figures of every case."""
import numpy as np
import pytest

import search_adversarial_util as A
from test_eps_bound import approx_scores, slack

RATIO_FLOOR = 0.28  # from the construction: (T - 16) / (2.5 d) less the small terms of eps; 0.25 is what a quartered slack tolerates


def _f16(a):
    return a.astype(np.float16).astype(np.float64)


def _norm(v):
    return float(np.linalg.norm(v.astype(np.float64)))


def _device_view(F):
    """mu, mq as the device computes them, whether the bias build runs, x' and dq, and 2 eps of every query."""
    mu, exact = A.colsum_mean(F.x)
    assert exact, "a column-sum partial is not exact in fp32"
    assert np.array_equal(mu, F.mu)
    xc = (F.x - mu).astype(np.float32)
    assert np.array_equal(xc, F.x_unc)                      # fl32(x - mu) is the uncentred fixture bit for bit
    mq = A.query_mean(F.q)
    xo = float(np.sqrt((F.x.astype(np.float64) ** 2).sum(axis=1).max())) * 1.0001
    lhs, rhs = _norm(mq) * 1.0001, 0.05 * xo
    if F.kind == "qmean":
        assert np.array_equal(mq, F.mq)
        assert lhs > 2.0 * rhs, (lhs, rhs)                  # query_mean_decide_kernel: bias build, by a factor >= 2
        use = True
    else:
        assert 2.0 * lhs < rhs, (lhs, rhs)                  # zeroed, by a factor >= 2
        mq, use = np.zeros_like(mq), False
    dq = (F.q - mq).astype(np.float32)
    norms = np.sqrt((xc.astype(np.float64) ** 2).sum(axis=1))
    assert norms.max() / norms.min() < 1.01                # eps scales with the MAXIMUM norm: no row may inflate it
    E = slack(F.d)
    Xc = float(norms.max()) * 1.0001
    qc = np.sqrt((dq.astype(np.float64) ** 2).sum(axis=1)) * 1.0001
    qo = np.sqrt((F.q.astype(np.float64) ** 2).sum(axis=1)) * 1.0001
    mqn = _norm(mq) * 1.0001 if use else 0.0
    eps2 = 2.0 * (E["rel_c"] * qc * Xc + E["acc_m"] * mqn * Xc + E["cen"] * qo * Xc + E["abs_c"] * (qc + Xc) + E["chain_o"] * qo * xo)
    return xc, dq, mq, eps2


def _check(name, F, knob_splits=0):
    from oracle import search_ref
    xc, dq, mq, eps2 = _device_view(F)
    uniq = F.n_unique
    q, dq, eps2, tie = F.q[:uniq], dq[:uniq], eps2[:uniq], F.tie_sign[:uniq]
    assert len(np.unique(F.x.view(np.uint32), axis=0)) == F.n  # distinct rows: no duplicate class to collapse
    # the oracle's top-k of every tie query: the victims (all tied exactly), ascending ids
    D, I = search_ref.flat_ip_topk_chain(F.x, q, F.k)
    for r in np.flatnonzero(tie):
        want = F.victims if tie[r] > 0 else F.neg_victims
        assert np.array_equal(I[r], want), (name, r)
        assert np.all(D[r] == D[r, 0])
    # s~ of every (query, row): b + fp16(dq) . fp16(x'), every product and partial sum exact for the tie queries
    bias = mq.astype(np.float64) @ xc.astype(np.float64).T
    S = (_f16(dq) @ _f16(xc).T + bias[None, :]).astype(np.float32)
    ratios, bands = [], []
    S_plan = A.plan_splits(F.n, len(F.q), F.k, knob_splits)
    for r in range(uniq):
        kth = np.partition(S[r], F.n - F.k)[F.n - F.k]
        band = int(np.count_nonzero(S[r] >= kth - eps2[r]))
        assert band <= A.BAND_MAX, (name, r, band)
        bands.append(band)
        per = -(-F.n // S_plan)                             # ... and in every corpus split on its own (its k-th best is lower)
        for s in range(S_plan):
            part = S[r, s * per:(s + 1) * per]
            if len(part) >= F.k:
                kp = np.partition(part, len(part) - F.k)[len(part) - F.k]
                assert np.count_nonzero(part >= kp - eps2[r]) <= A.BAND_MAX, (name, r, s)
        if not tie[r]:
            continue
        vic, imp = (F.victims, F.impostors) if tie[r] > 0 else (F.neg_victims, F.neg_impostors)
        worst = S[r, vic].min()
        assert kth == S[r, imp].min() and np.all(S[r, imp] == kth)   # the k best approximate scores are impostors'
        # the same figures under the accumulation orders of test_eps_bound.py (the MFMA's own order is unspecified)
        for row, val in ((vic[0], S[r, vic[0]]), (imp[-1], kth)):
            for st in approx_scores(dq[r], xc[row], float(bias[row])):
                assert st == float(val), (name, r, row)
        ratio = float(kth - worst) / float(eps2[r])
        assert ratio >= RATIO_FLOOR, (name, r, ratio)
        ratios.append(ratio)
    print("%-44s S=%d  deficit / 2 eps = %.3f .. %.3f   band rows = %d .. %d" % (name, S_plan, min(ratios), max(ratios), min(bands),
                                                                                 max(bands)))
    return min(ratios)


@pytest.mark.parametrize("name", sorted(A.CASES))
def test_fixture_is_adversarial(name):
    _check(name, A.fixture(name))


def _split_of(F, ids, splits, window):
    """Corpus split that scans a row: windows of `window` tiles (0: one window), each dealt out to the splits in runs."""
    n_tiles = F.n // 256
    wt = window if 0 < window <= n_tiles else n_tiles
    ws = -(-wt // splits)
    return (ids // 256) % (ws * splits) // ws


@pytest.mark.parametrize("splits,window,variant", sorted(A.SPLIT_CASES))
def test_split_matrix_fixture(splits, window, variant):
    """The tiled query block keeps the mean query below the 0.05 rule and the planner at the requested split count; the rows
    lie in the splits the variant is about."""
    F = A.build(**A.SPLIT_CASES[(splits, window, variant)])
    assert A.plan_splits(F.n, len(F.q), F.k, splits) == splits
    _check("splits%d_window%d_%s" % (splits, window, variant), F, splits)
    sv, si = _split_of(F, F.victims, splits, window), _split_of(F, F.impostors, splits, window)
    if variant == "k200_shuffled":       # every split holds victims and impostors, none holds k impostors
        assert set(sv) == set(si) == set(range(splits))
    elif variant == "k10_dense_shuffled":  # every split holds more than k impostors
        assert np.bincount(si, minlength=splits).min() > F.k and len(set(sv)) > 1
    elif window:                         # ordered: all impostors in one split, all victims in another
        assert len(set(sv)) == len(set(si)) == 1 and sv[0] != si[0]


def test_no_prune_case_meets_no_prune():
    """'late' placement at n = 4096, k = 10: two corpus splits of 8 tiles, scheduled prunes after tiles 2, 3, 4 and 6 of a
    split, victims and impostors in its tile 8 -- inserted under a threshold the fillers set, pruned by nobody."""
    F = A.fixture("noprune_d128_n4096_k10")
    assert A.plan_splits(F.n, len(F.q), F.k) == 2
    tiles = F.n // 256 // 2
    prunes = A.scheduled_prunes(F.k, tiles)
    last = prunes[-1]
    for ids in (F.victims, F.impostors, F.neg_victims, F.neg_impostors):
        assert np.all((ids // 256) % tiles + 1 > last)
    # ... and no list fills up in between (an unscheduled prune): a prune leaves a list of fillers k rows and one score
    # level of them (< 256 rows), the tiles up to the next prune or the end add 256 each
    gaps = np.diff([0] + prunes + [tiles])
    assert 256 + 256 * int(gaps.max()) <= 2048 - 256
