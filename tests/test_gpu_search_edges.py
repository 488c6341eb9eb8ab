"""Edges of the search entry points no other test reaches, each against oracle/search_ref.py bit for bit: more duplicate
classes than a search image collapses (and a class that starts at row 0), ance_topk_merge on padded / empty / full-size /
tied / high-id parts, ance_ip_score_rows on out-of-range ids, empty ranges and long candidate lists.  Needs an MI355X."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NEG_FILL = np.float32(-3.4028234663852886e38)


@pytest.fixture(autouse=True)
def _knobs_follow_the_environment():
    yield
    from ance_amd import _lib
    _lib.reload_env()


# ---- duplicate classes ----------------------------------------------------------------------------------------------------
def test_more_duplicate_classes_than_the_image_collapses():
    """Six classes of bit-identical rows, each 6 % of a 40,000-row shard (2,400 members: more than the 1,024 member ids an
    image keeps per class), one of them starting at row 0.  The image collapses four (DEDUP_MAXC) and WHICH four is a race
    between the threads that find them: whatever the outcome, the lists are the oracle's -- twice, from two builds."""
    from ance_amd import _lib
    from ance_amd.index import FlatIPIndex
    from oracle import search_ref, synth
    rng = np.random.default_rng(71)
    n, d = 40000, 128
    x = synth.ln_rows(rng, n, d=d)
    v = synth.ln_rows(rng, 6, d=d)
    owner = rng.permutation(n)
    for c in range(6):
        x[owner[c * 2400:(c + 1) * 2400]] = v[c]
    x[0] = v[2]                                    # this class's smallest id -- its representative -- is row 0
    rows = rng.integers(0, n, 12)
    q = np.concatenate([v, -v[:1], (0.6 * v[0] + 0.8 * v[1])[None], (v[2] + v[5])[None], (v[3] + 0.5 * synth.ln_rows(rng, 1, d=d)[0])[None],
                        x[rows], synth.ln_rows(rng, 12, d=d)]).astype(np.float32)
    _lib.reload_env()
    for k in (200, 1000):
        Do, Io = search_ref.flat_ip_topk_chain(x, q, k)
        for attempt in range(2):
            idx = FlatIPIndex(d)
            idx.add(x)
            D, I = idx.search(q, k)
            assert np.array_equal(I, Io), (k, attempt)
            assert np.array_equal(D, Do), (k, attempt)
        # a class vector as the query: the whole list is that class, ascending ids, row 0 first for its class
        for c in range(6):
            assert np.all(np.diff(Io[c]) > 0) and np.all(x[Io[c]] == v[c])
        assert Io[2, 0] == 0


# ---- ance_topk_merge ------------------------------------------------------------------------------------------------------
def _parts(rng, P, nq, k, fill, id_lo=0, id_hi=1 << 20, levels=None):
    """Canonical lists [P, nq, k]: part p of query r holds fill[p] (<= k) entries, ids distinct over the parts of a query,
    scores drawn from `levels` values when given (ties inside and across parts), padded with -1 / -FLT_MAX."""
    D = np.full((P, nq, k), NEG_FILL, np.float32)
    I = np.full((P, nq, k), -1, np.int64)
    for r in range(nq):
        ids = id_lo + rng.choice(id_hi - id_lo, size=int(sum(fill)), replace=False).astype(np.int64)
        o = 0
        for p in range(P):
            m = fill[p]
            i = ids[o:o + m]
            o += m
            s = (rng.integers(0, levels, m) / 8.0 - 3.0 if levels else rng.standard_normal(m)).astype(np.float32)
            order = np.lexsort((i, -s.astype(np.float64)))
            D[p, r, :m], I[p, r, :m] = s[order], i[order]
    return D, I


def _merge_check(D, I):
    import torch
    from ance_amd.index import topk_merge_device
    from oracle import search_ref
    Dm, Im = topk_merge_device(torch.from_numpy(D).cuda(), torch.from_numpy(I).cuda())
    Do, Io = search_ref.topk_merge(D, I, D.shape[2])
    assert np.array_equal(Im.cpu().numpy(), Io)
    assert np.array_equal(Dm.cpu().numpy(), Do)
    return Do, Io


def test_merge_padded_and_empty_parts():
    """Shards with fewer than k rows: parts that end in -1 / -FLT_MAX padding, one part empty, fewer than k entries in all."""
    rng = np.random.default_rng(72)
    _merge_check(*_parts(rng, 4, 7, 50, [50, 13, 0, 1]))
    Do, Io = _merge_check(*_parts(rng, 3, 5, 40, [9, 0, 17]))     # 26 < k entries: the merged list is padded too
    assert np.all(Io[:, 26:] == -1) and np.all(Do[:, 26:] == NEG_FILL) and np.all(Io[:, :26] >= 0)
    _merge_check(*_parts(rng, 2, 3, 10, [0, 0]))                  # nothing at all


def test_merge_one_part_and_odd_sizes():
    rng = np.random.default_rng(73)
    _merge_check(*_parts(rng, 1, 9, 200, [200]))                  # P = 1: the list itself
    _merge_check(*_parts(rng, 1, 4, 1, [1]))
    _merge_check(*_parts(rng, 3, 6, 100, [100, 100, 100]))        # P k = 300, no power of two
    _merge_check(*_parts(rng, 7, 3, 333, [333, 5, 333, 0, 332, 333, 100]))


def test_merge_at_its_size_limit():
    """P k = 16,384 exactly (the whole LDS sort), and the refusal one entry above."""
    import torch
    from ance_amd import _lib
    from ance_amd.index import topk_merge_device
    rng = np.random.default_rng(74)
    _merge_check(*_parts(rng, 16, 3, 1024, [1024] * 16))
    _merge_check(*_parts(rng, 16, 2, 1024, [1024] * 16, levels=40))
    D = torch.zeros((5, 1, 3277), dtype=torch.float32, device="cuda")     # 5 x 3277 = 16,385
    with pytest.raises(_lib.AnceLibraryError):
        topk_merge_device(D, torch.zeros((5, 1, 3277), dtype=torch.int64, device="cuda"))


def test_merge_ties_across_parts_and_high_ids():
    """Equal scores in different parts come out in ascending id order; ids in [2^31, 2^32) survive the packed keys."""
    rng = np.random.default_rng(75)
    D, I = _parts(rng, 5, 8, 64, [64, 64, 30, 64, 1], levels=6)
    Do, Io = _merge_check(D, I)
    same = Do[:, 1:] == Do[:, :-1]
    assert same.sum() > 100 and np.all(Io[:, 1:][same] > Io[:, :-1][same])
    D, I = _parts(rng, 4, 6, 100, [100, 7, 100, 100], id_lo=1 << 31, id_hi=1 << 32, levels=12)
    Do, Io = _merge_check(D, I)
    assert Io.min() >= 1 << 31 and Io.max() < 1 << 32
    lo = _parts(rng, 2, 3, 20, [20, 20], id_lo=(1 << 31) - 20, id_hi=(1 << 31) + 20, levels=3)   # ids on both sides of 2^31
    _merge_check(*lo)


# ---- ance_ip_score_rows ---------------------------------------------------------------------------------------------------
def _score_rows(x, q, rows, offsets):
    """Scores of the C entry point, written into the middle of a poisoned buffer; asserts the poison is untouched."""
    import torch
    from ance_amd import _lib
    guard = 64
    xd, qd = torch.from_numpy(x).cuda(), torch.from_numpy(q).cuda()
    rd, od = torch.from_numpy(rows).cuda(), torch.from_numpy(offsets).cuda()
    buf = torch.full((guard + len(rows) + guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    base = buf.data_ptr() + 4 * guard
    rc = _lib.lib().ance_ip_score_rows(ctypes.c_void_p(xd.data_ptr()), x.shape[0], ctypes.c_void_p(qd.data_ptr()), q.shape[0], x.shape[1],
                                       ctypes.c_void_p(rd.data_ptr()), ctypes.c_void_p(od.data_ptr()), ctypes.c_void_p(base),
                                       _lib.current_stream_ptr())
    _lib.check(rc, "ance_ip_score_rows")
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert np.all(out[:guard] == 0x5A5A5A5A) and np.all(out[guard + len(rows):] == 0x5A5A5A5A)
    return out[guard:guard + len(rows)].view(np.float32)


@pytest.mark.parametrize("d", [4, 768, 2048])
def test_score_rows_edges(d):
    """Candidate ids -1 and n score -inf and touch nothing else; a query with an empty range between two non-empty ones;
    700 candidates for one query (a thread walks several); scores bit-identical to the chain oracle."""
    from oracle import search_ref
    rng = np.random.default_rng(76 + d)
    n, nq = 3000, 6
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    counts = [300, 0, 700, 1, 0, 257]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rows = rng.integers(0, n, size=int(offsets[-1])).astype(np.int64)
    bad = {3: -1, 299: n, 300: n, 650: -1, 999: -1, 1000: n + 5, int(offsets[-1]) - 1: -7}   # first / last of a range, mid-list
    for j, r in bad.items():
        rows[j] = r
    rows[5], rows[310] = 0, n - 1                   # the valid ends of the id range
    s = _score_rows(x, q, rows, offsets)
    S = search_ref.ip_scores_chain(x, q)
    for qi in range(nq):
        for j in range(int(offsets[qi]), int(offsets[qi + 1])):
            if j in bad:
                assert s[j] == -np.inf, j
            else:
                assert s[j].view(np.uint32) == S[qi, rows[j]].view(np.uint32), (qi, j)
