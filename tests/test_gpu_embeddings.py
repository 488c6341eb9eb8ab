"""The trainable embeddings (ance_amd/embeddings.py -> csrc/embed_train.hip) on the GPU against the fp64 restatement of
tests/embeddings_util.py and the reference's own tensors (tests/golden/embeddings*.npz).

Bound, per tensor:  max |got - fp64| <= max(4 x D_ref, 16 ulp32 of the fp64 tensor's largest magnitude), D_ref the eager fp32
expression's own distance from fp64: the fixture's recorded ones for the golden cases, the torch CPU evaluation of the same inputs and
the same mask for the seeded ones.  Every measured distance is printed: delta, reference, ratio, bound.  The word table's gradient is
compared on the rows that occur; every other row must be exactly zero."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import embeddings_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN32 = 0x7FC00ABC   # the sentinel: a NaN with a recognisable payload
SEED = 0x5EED0123456789AB
KERNELS = ("embed_fwd_kernel", "embed_bwd_kernel", "colsum_tree_kernel", "seg_piece_kernel", "seg_join_kernel")
BACKWARD_LAUNCHES = 4   # include/ance_amd.h: the row kernel, the column-sum tree, the pieces, the joins


def _dev(x, grad=False):
    if x is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t.requires_grad_(True) if grad else t


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check(tag, got, want, ref_err, names=U.NAMES):
    bad = []
    for n in names:
        d = float(np.abs(np.asarray(got[n], np.float64) - want[n]).max())
        b = U.bound(ref_err[n], np.abs(want[n]).max())
        print("%-52s %-6s max|delta| %.3e  reference %.3e  ratio %6.2f  bound %.3e" % (tag, n, d, ref_err[n], d / max(ref_err[n], 1e-300), b))
        if not d <= b:
            bad.append((n, d, b))
    assert not bad, (tag, bad)


def _run(ids, types, tables, eps, dy, mode="absolute", pad=None, p=0.0, training=True, ids_dtype=torch.int64, dev_tables=None):
    """One forward + backward through ance_amd.embeddings.bert_embeddings.  dict(y [T, H], dword (rows that occur), dword_rest_zero,
    dpos, dtype, dgamma, dbeta) and the leaves."""
    from ance_amd.embeddings import bert_embeddings
    tw, tp, tt, tg, tb = dev_tables if dev_tables is not None else tuple(_dev(t, True) for t in tables)
    for t in (tw, tp, tt, tg, tb):
        t.grad = None
    y = bert_embeddings(_dev(ids).to(ids_dtype), tw, tp, tt, tg, tb, eps, None if types is None else _dev(types).to(ids_dtype), mode, pad, p, training)
    y.backward(_dev(dy).view(y.shape))
    rows = torch.from_numpy(np.unique(U.clamp_ids(ids, tw.shape[0]))).to(DEV)
    dword = tw.grad
    rest_zero = bool(torch.count_nonzero(dword) == torch.count_nonzero(dword[rows]))
    return dict(y=_np(y).reshape(-1, y.shape[-1]), dword=_np(dword[rows]), dword_rest_zero=rest_zero, dpos=_np(tp.grad), dtype=_np(tt.grad),
                dgamma=_np(tg.grad), dbeta=_np(tb.grad))


def _reference(ids, types, tables, eps, dy, mode, pad, p=0.0, offset=0):
    """The fp64 restatement and the eager fp32 expression's distances under the mask of (SEED, offset): on the CPU."""
    H = tables[0].shape[1]
    keep = U.tail_keep_mask(p, SEED, offset, ids.size, H) if p > 0 else None
    want = U.embed_fp64(ids, types, *tables, eps, dy, mode, pad, keep, p)
    return keep, want, U.distances(U.embed_eager_fp32(ids, types, *tables, eps, dy, mode, pad, keep, p), want)


@functools.lru_cache(maxsize=None)
def _tables(tag, H, vocab=1000, max_pos=514, n_types=2):
    return U.embed_inputs(tag, H, vocab, max_pos, n_types)


def _chunk():
    from ance_amd import _lib
    C = _lib.EMBED_SEGMENT_CHUNK   # the segmented sum's chunk, as the library states it
    assert _lib.lib().ance_embed_segment_chunk() == C
    return C


# ------------------------------------------------------------------------------------------------------------------------ golden
@functools.lru_cache(maxsize=None)
def _golden_device_tables(case, golden_dir):
    """The real-vocabulary tables of a tower, on the device once per module."""
    m, t = U.load_golden(golden_dir, case)
    tables = U.golden_tables(m)
    return m, t, tables, tuple(_dev(x, True) for x in tables)


@pytest.mark.parametrize("case", U.GOLDEN_CASES)
def test_golden_embeddings(golden_dir, case):
    """Both towers' own tensors at their real vocabulary sizes: y and the five gradients against fp64 within the bound set by the
    reference's own fp32-to-fp64 distance and by the eager expression's distance on the committed inputs, and next to the reference's
    fp32 results."""
    m, t, tables, dev_tables = _golden_device_tables(case, golden_dir)
    L = m["L"]
    want = U.embed_fp64(t["ids"], t["types"], *tables, m["eps"], t["dy"], m["position_mode"], m["padding_idx"])
    types = None if case == "rdot" else t["types"]   # the towers pass no type ids; zeros are the same thing
    got = _run(t["ids"], types, tables, m["eps"], t["dy"], m["position_mode"], m["padding_idx"], 0.1, False, dev_tables=dev_tables)   # eval mode
    assert got["dword_rest_zero"] and np.all(got["dpos"][L + 2:] == 0)
    got["dpos"], want["dpos"] = got["dpos"][:L + 2], want["dpos"][:L + 2]
    _check("golden %s" % case, got, want, m["ref_err"])
    _check("golden %s, same inputs" % case, got, want, m["same_inputs"])
    for n in U.NAMES:   # the reference's fp32 tensors: both are within the bound of fp64, so within twice it of each other
        d = float(np.abs(got[n].astype(np.float64) - t[n]).max())
        b = 2 * U.bound(m["ref_err"][n], np.abs(want[n]).max())
        print("golden %s %-6s vs the reference's fp32 %.3e  bound %.3e" % (case, n, d, b))
        assert d <= b, (n, d, b)


# ------------------------------------------------------------------------------------------------------------------------ row and duplicate sweep
SWEEP_VOCAB = 2100
SWEEP_SHAPES = lambda R: ((1, 1), (3, 5), (2, 8), (1, 17), (1, 3 * R + 5), (5, (130 * R + 5) // 5))   # noqa: E731


def _place(tag, sorted_keys):
    """The multiset `sorted_keys` (ascending: its order IS the sorted order the kernels will see) dealt to the rows by a seeded
    permutation."""
    order = np.argsort(U.seeded_ids(tag + ".perm", (len(sorted_keys),), 0, 1 << 30), kind="stable")
    out = np.empty(len(sorted_keys), np.int64)
    out[order] = sorted_keys
    return out


def _run_lengths(tag, T, counts, vocab):
    """T ids whose sorted order starts with runs of the given (key, count), cut off at T, and goes on with seeded ids above them --
    ids 0 and vocab - 1 among them."""
    keys = np.concatenate([np.full(c, k, np.int64) for k, c in counts])[:T]
    rest = T - len(keys)
    if rest > 0:
        tail = np.sort(U.seeded_ids(tag + ".tail", (rest,), 100, vocab))
        tail[-1] = vocab - 1
        keys = np.concatenate([keys, tail])
    return _place(tag, np.sort(keys))


def _sweep_ids(pattern, n_seq, L, C, vocab):
    T = n_seq * L
    tag = "sweep.%s.%d" % (pattern, T)
    if pattern == "distinct":
        ids = _place(tag, np.arange(T) % vocab)            # T <= vocab: every id once; ids 0 and T - 1 occur
    elif pattern == "equal":
        ids = np.full(T, 7, np.int64)                       # one key owns every row and crosses every chunk boundary
    elif pattern == "straddle":
        # sorted positions: key 0 fills 0 .. 29, then runs of C - 1, C, C + 1 and 3 C + 5, each across a chunk boundary
        ids = _run_lengths(tag, T, ((0, 30), (10, C - 1), (20, C), (30, C + 1), (40, 3 * C + 5)), vocab)
    else:
        # aligned: a run that IS a chunk, one that is two whole chunks, a single row, a run that ends with its chunk, one that starts one
        ids = _run_lengths(tag, T, ((0, C), (10, 2 * C), (20, 1), (30, C - 1), (40, C + 1)), vocab)
    return ids.reshape(n_seq, L)


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("H", [768, 1024])
def test_row_and_duplicate_sweep(H, p):
    """Row counts around the 16-row workgroup and the reducer's tree; ids all distinct, all equal (with a ONE-row type table: its
    gradient is the column sum), and with keys of C - 1, C, C + 1 and 3 C + 5 rows placed across and onto the chunk boundaries of the
    sorted order; ids 0 and vocab - 1 occur; type ids mixed 0 / 1."""
    from ance_amd import _lib, attention as T
    R, C = _lib.LAYER_TAIL_ROWS_PER_WORKGROUP, _chunk()
    rows_seen = set()
    for n_seq, L in SWEEP_SHAPES(R):
        n = n_seq * L
        rows_seen.add(n)
        patterns = ("distinct", "equal", "straddle", "aligned") if n >= C else ("distinct", "equal")
        for pattern in patterns:
            one_type = pattern == "equal"
            tables = _tables("sweep.%d.%d" % (H, one_type), H, SWEEP_VOCAB, 514, 1 if one_type else 2)
            ids = _sweep_ids(pattern, n_seq, L, C, SWEEP_VOCAB)
            if pattern in ("straddle", "aligned") and n > 6 * C:
                assert ids.min() == 0 and ids.max() == SWEEP_VOCAB - 1
                assert {C - 1, C, C + 1, 3 * C + 5 if pattern == "straddle" else 2 * C} <= set(np.bincount(ids.reshape(-1)).tolist())
            types = None if one_type else U.seeded_ids("sweep.tt.%d" % n, ids.shape, 0, 2)
            dy = U.embed_dy("sweep.%d" % H, n, H)
            keep, want, ref = _reference(ids, types, tables, 1e-5, dy, "absolute", None, p)
            T.manual_seed(SEED)   # offset 0
            got = _run(ids, types, tables, 1e-5, dy, "absolute", None, p)
            assert got["dword_rest_zero"] and np.all(got["dpos"][L:] == 0)
            _check("H %d p %.1f rows %d (%d x %d) %s" % (H, p, n, n_seq, L, pattern), got, want, ref)
    assert rows_seen == {1, R - 1, R, R + 1, 3 * R + 5, 130 * R + 5}


# ------------------------------------------------------------------------------------------------------------------------ positions
def test_positions_and_padding_rows():
    """roberta mode at L = 512 with max_pos 514 (the position reaches 513), interior pads, a sequence of pads only, a length-1
    sequence; absolute mode at L = 512 = max_pos.  The word row and, in roberta mode, the position row of padding_idx get exactly
    zero gradient although dy is non-zero there."""
    H, vocab, pad, L = 768, 1000, 1, 512
    ids = U.seeded_ids("pos", (4, L), 3, vocab)
    ids[1, [0, 5, 6, 100, 511]] = pad      # interior pads, a leading and a trailing one
    ids[2, :] = pad                         # pads only
    ids[3, 300:] = pad                      # right padding
    dy = U.embed_dy("pos", ids.size, H)
    assert np.abs(dy.reshape(4, L, H)[ids == pad]).max() > 0   # the gradient that arrives at the pad rows is not zero
    for mode, max_pos in (("roberta", 514), ("absolute", 512)):
        tables = _tables("pos", H, vocab, max_pos, 2)
        types = U.seeded_ids("pos.tt", ids.shape, 0, 2)
        keep, want, ref = _reference(ids, types, tables, 1e-5, dy, mode, pad)
        if mode == "roberta":
            assert want["positions"][0, L - 1] == 513 and np.all(want["positions"][2] == pad) and want["positions"][1, 7] == pad + 5
        got = _run(ids, types, tables, 1e-5, dy, mode, pad)
        _check("%s L 512 max_pos %d" % (mode, max_pos), got, want, ref)
        pad_row = np.flatnonzero(np.unique(ids) == pad)
        assert np.all(_bits(got["dword"][pad_row]) == 0), "the word table's padding row must stay exactly zero"
        assert got["dword_rest_zero"]
        if mode == "roberta":
            assert np.all(_bits(got["dpos"][pad]) == 0) and np.all(got["dpos"][0] == 0)
            assert np.abs(got["dpos"][513]).max() > 0
        else:
            assert np.abs(got["dpos"][pad]).max() > 0 and np.abs(got["dpos"][511]).max() > 0
    # a length-1 sequence: one row; a pad alone (roberta: position = padding_idx) and a token alone
    tables = _tables("pos", H, vocab, 514, 2)
    for tok in (pad, 17):
        one = np.array([[tok]], np.int64)
        keep, want, ref = _reference(one, None, tables, 1e-5, dy[:1], "roberta", pad)
        assert want["positions"][0, 0] == (pad if tok == pad else pad + 1)
        _check("roberta L 1 id %d" % tok, _run(one, None, tables, 1e-5, dy[:1], "roberta", pad), want, ref)


# ------------------------------------------------------------------------------------------------------------------------ the clamp
def test_out_of_range_ids_are_read_as_the_nearest_valid_one():
    """Ids -1 and vocab and a type id 2 with a 2-row table: the forward gives the bits of the clamped ids, the gradients land in the
    clamped rows.  (The clamp is the first statement of every kernel that takes an id: this checks the documented behaviour.)"""
    H, vocab = 768, 1000
    tables = _tables("clamp", H, vocab, 514, 2)
    ids = U.seeded_ids("clamp", (3, 40), 2, vocab - 2)
    types = U.seeded_ids("clamp.tt", ids.shape, 0, 2)
    ids[0, 3], ids[1, 7], ids[2, 39] = -1, vocab, vocab
    ids[0, 4], ids[1, 8] = 0, vocab - 1            # the clamped rows also occur as themselves
    types[0, 3], types[2, 5] = 2, 2
    dy = U.embed_dy("clamp", ids.size, H)
    cl_ids, cl_types = np.clip(ids, 0, vocab - 1), np.clip(types, 0, 1)
    for mode, pad in (("absolute", None), ("roberta", 1)):
        keep, want, ref = _reference(cl_ids, cl_types, tables, 1e-5, dy, mode, pad)
        got, clamped = _run(ids, types, tables, 1e-5, dy, mode, pad), _run(cl_ids, cl_types, tables, 1e-5, dy, mode, pad)
        assert np.array_equal(_bits(got["y"]), _bits(clamped["y"]))
        _check("clamp %s" % mode, got, want, ref)
        assert got["dword_rest_zero"] and np.abs(got["dword"][0]).max() > 0 and np.abs(got["dword"][-1]).max() > 0
        for n in ("dpos", "dgamma", "dbeta"):   # nothing but the grouping of the clamped rows can differ
            assert np.array_equal(_bits(got[n]), _bits(clamped[n])), n


# ------------------------------------------------------------------------------------------------------------------------ hard rows
@pytest.mark.parametrize("eps", [1e-5, 1e-12])
def test_hard_rows_for_the_layer_norm(eps):
    H, vocab, n_seq, L = 768, 64, 3, 7
    word, pos, typ, g, be = _tables("hard", H, vocab, 16, 2)
    ids, types = U.seeded_ids("hard", (n_seq, L), 0, vocab), U.seeded_ids("hard.tt", (n_seq, L), 0, 2)
    dy = U.embed_dy("hard", n_seq * L, H)

    def both(tag, tables, types=types):
        keep, want, ref = _reference(ids, types, tables, eps, dy, "absolute", None)
        got = _run(ids, types, tables, eps, dy, "absolute", None)
        _check("%s eps %g" % (tag, eps), got, want, ref)
        return got

    # mean 100, spread 0.01: E[v^2] - mean^2 in fp32 has no correct digit here
    both("mean 100 spread 0.01", ((100.0 + 0.01 * word).astype(np.float32), pos * np.float32(0.01), typ * np.float32(0.01), g, be))
    # sums that are exactly constant along the row: xhat is exactly 0 and y is beta, bit for bit.  The constants have short mantissas,
    # so every partial sum of 768 of them is exact in fp32 in any order and the mean is the constant itself.
    cw = (np.arange(vocab, dtype=np.float32)[:, None] - 7.0) * np.float32(0.375) + np.zeros((vocab, H), np.float32)
    cp = np.arange(16, dtype=np.float32)[:, None] * np.float32(0.25) + np.zeros((16, H), np.float32)
    ct = np.array([[0.5], [-1.5]], np.float32) + np.zeros((2, H), np.float32)
    got = both("constant rows", (cw, cp, ct, g, be))
    assert np.array_equal(_bits(got["y"]), _bits(np.broadcast_to(be, (n_seq * L, H)))), "y must equal beta bit for bit"
    assert np.all(got["dgamma"] == 0)
    # a quarter of gamma exactly 0, beta nonzero: xhat cannot be taken from (y - beta) / gamma
    g0 = g.copy()
    g0[::4] = 0.0
    assert np.all(be != 0)
    got = both("gamma with zeros", (word, pos, typ, g0, be))
    assert np.all(np.isfinite(got["dgamma"])) and np.abs(got["dgamma"][::4]).max() > 0
    got = both("gamma all zero", (word, pos, typ, np.zeros_like(g), be))
    assert np.all(got["dword"] == 0) and np.all(got["dpos"] == 0) and np.abs(got["dgamma"]).max() > 0


# ------------------------------------------------------------------------------------------------------------------------ dropout
def test_dropout_mask_stream_and_seed():
    from ance_amd import attention as T
    H, n_seq, L, p = 1024, 5, 9, 0.5
    tables = _tables("dropout", H)
    ids, types = U.seeded_ids("dropout", (n_seq, L), 0, 1000), U.seeded_ids("dropout.tt", (n_seq, L), 0, 2)
    dy = U.embed_dy("dropout", n_seq * L, H)
    keep, want, ref = _reference(ids, types, tables, 1e-5, dy, "absolute", None, p, 0)
    assert np.all(U.embed_fp64(ids, types, *tables, 1e-5, dy)["y"] != 0)      # a kept element is never 0
    T.manual_seed(SEED)
    before = dict(T.dropout_state.offsets)
    r0 = _run(ids, types, tables, 1e-5, dy, p=p)                                # offset 0
    assert T.dropout_state.offsets[0] == before.get(0, 0) + 1                   # exactly one per dropping call
    assert np.array_equal(r0["y"] != 0, keep), "the kept set is the restated one, element for element"
    _check("dropout p 0.5 offset 0", r0, want, ref)
    r1 = _run(ids, types, tables, 1e-5, dy, p=p)                                # offset 1
    assert T.dropout_state.offsets[0] == before.get(0, 0) + 2
    keep1, want1, ref1 = _reference(ids, types, tables, 1e-5, dy, "absolute", None, p, 1)
    assert np.array_equal(r1["y"] != 0, keep1) and not np.array_equal(keep, keep1)
    _check("dropout p 0.5 offset 1", r1, want1, ref1)
    T.manual_seed(SEED)
    r2 = _run(ids, types, tables, 1e-5, dy, p=p)
    for k in U.NAMES:
        assert np.array_equal(_bits(r0[k]), _bits(r2[k])), k
    plain = _run(ids, types, tables, 1e-5, dy)
    at = dict(T.dropout_state.offsets)
    for kw in (dict(p=p, training=False), dict(p=0.0, training=True)):
        r = _run(ids, types, tables, 1e-5, dy, **kw)
        for k in U.NAMES:
            assert np.array_equal(_bits(plain[k]), _bits(r[k])), (kw, k)
    assert T.dropout_state.offsets == at                                        # no draw, no counter advance
    # one stream with the layer tail: its dropout call takes the next pair
    from ance_amd.layers import dropout_add_layer_norm
    x = torch.zeros(4, 768, device=DEV)
    dropout_add_layer_norm(x, None, x, torch.ones(768, device=DEV), torch.zeros(768, device=DEV), 1e-5, 0.1, True)
    assert T.dropout_state.offsets[0] == at[0] + 1


# ------------------------------------------------------------------------------------------------------------------------ determinism
def _traced_kernels(fn):
    """Names of the kernels of one call, from torch.profiler."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events()
            if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]


def test_deterministic_capturable_and_never_synchronises():
    """Two runs give the same bits; forward + backward are captured in a graph -- torch's device sort included -- and replayed to the
    eager run's bits; no call waits for the device; one kernel forward, BACKWARD_LAUNCHES of this library's backward (the sorts are
    torch's and are counted and named apart)."""
    from ance_amd import attention as T
    from ance_amd.embeddings import bert_embeddings
    H, vocab, pad, n_seq, L = 768, 1000, 1, 6, 70
    tables = [_dev(t) for t in _tables("capture", H, vocab, 514, 2)]
    ids = U.seeded_ids("capture", (n_seq, L), 0, 40)      # forty ids over 420 rows: every key is a run of several rows
    ids[2, 10:30] = pad
    tid, ttt = _dev(ids).to(torch.int32), _dev(U.seeded_ids("capture.tt", ids.shape, 0, 2)).to(torch.int32)
    tdy = _dev(U.embed_dy("capture", n_seq * L, H)).view(n_seq, L, H)

    def forward(p, leaves):
        return bert_embeddings(tid, *leaves, 1e-5, ttt, "roberta", pad, p, True)

    def step(p):
        leaves = [t.clone().requires_grad_(True) for t in tables]
        y = forward(p, leaves)
        y.backward(tdy)
        return [y.detach()] + [t.grad for t in leaves]

    for p in (0.0, 0.1):
        T.manual_seed(5)
        e1 = [t.clone() for t in step(p)]
        T.manual_seed(5)
        e2 = [t.clone() for t in step(p)]
        torch.cuda.synchronize()
        for a, c in zip(e1, e2):
            assert torch.equal(a.view(torch.int32), c.view(torch.int32))
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
            for a, c in zip(e1, outs):
                assert torch.equal(a.view(torch.int32), c.view(torch.int32))
    # launches
    leaves = [t.clone().requires_grad_(True) for t in tables]
    held = {}
    fwd = _traced_kernels(lambda: held.__setitem__("y", forward(0.1, leaves)))
    bwd = _traced_kernels(lambda: held["y"].backward(tdy))
    ours = lambda names: [n for n in names if any(k in n for k in KERNELS)]   # noqa: E731
    print("forward kernels:", fwd)
    print("backward kernels of this library:", ours(bwd))
    print("backward kernels of torch (three stable sorts, zero fills, the statistics' copy):", [n for n in bwd if n not in ours(bwd)])
    assert len(fwd) == 1 and "embed_fwd_kernel" in fwd[0], fwd
    assert len(ours(bwd)) == BACKWARD_LAUNCHES, ours(bwd)
    assert [k for k in KERNELS[1:] if sum(k in n for n in bwd) != 1] == [], bwd


# ------------------------------------------------------------------------------------------------------------------------ the C ABI
class _Guarded:
    """A flat window of 4-byte words inside a buffer of sentinels, guards in front and behind (each a multiple of 16 bytes)."""

    def __init__(self, words, x=None, dtype=torch.float32, guard=64, fill=None):
        self.words, self.guard, self.dtype = words, guard, dtype
        self.buf = torch.full((words + 2 * guard,), NAN32, dtype=torch.int32, device=DEV)
        if x is not None:
            self.buf[guard:guard + words] = _dev(np.ascontiguousarray(x).reshape(-1)).view(torch.int32)
        elif fill is not None:
            self.buf[guard:guard + words] = fill

    @property
    def ptr(self):
        return self.buf[self.guard:].data_ptr()

    def window(self, shape=None):
        w = self.buf[self.guard:self.guard + self.words].view(self.dtype)
        return _np(w) if shape is None else _np(w).reshape(shape)

    def guards_intact(self):
        bits, g = _np(self.buf), self.guard
        return bool(np.all(bits[:g] == NAN32) and np.all(bits[g + self.words:] == NAN32))

    def untouched(self):
        return bool(np.all(_np(self.buf) == NAN32))


def _c_call(mode, pad, p=0.5, offset=3, n_seq=3, L=45, H=768, vocab=300, max_pos=64):
    from ance_amd import _lib
    L_ = _lib.lib()
    tables = _tables("cabi", H, vocab, max_pos, 2)
    ids = U.seeded_ids("cabi", (n_seq, L), 0, 60)
    ids[1, 4:9] = 1
    types = U.seeded_ids("cabi.tt", (n_seq, L), 0, 2)
    T_ = n_seq * L
    dy = U.embed_dy("cabi", T_, H)
    keep, want, ref = _reference(ids, types, tables, 1e-5, dy, mode, pad, p, offset)
    ins = dict(ids=_dev(ids.astype(np.int32)), types=_dev(types.astype(np.int32)), dy=_dev(dy), tables=[_dev(t) for t in tables])
    ws_bytes = L_.ance_embed_workspace_bytes(T_, H)
    bufs = dict(y=_Guarded(T_ * H), positions=_Guarded(T_, dtype=torch.int32), ws=_Guarded(ws_bytes // 4), dword=_Guarded(vocab * H, fill=0),
                dpos=_Guarded(max_pos * H, fill=0), dtype=_Guarded(2 * H, fill=0), dgamma=_Guarded(H), dbeta=_Guarded(H))
    tw, tp, tt, tg, tb = ins["tables"]
    a = _lib.AnceEmbedArgs(ids=ins["ids"].data_ptr(), type_ids=ins["types"].data_ptr(), word=tw.data_ptr(), pos=tp.data_ptr(), type=tt.data_ptr(),
                           gamma=tg.data_ptr(), beta=tb.data_ptr(), y=bufs["y"].ptr, positions=bufs["positions"].ptr, n_seq=n_seq, L=L, H=H,
                           vocab=vocab, max_pos=max_pos, n_types=2, position_mode=_lib.EMBED_POSITION_MODES[mode],
                           padding_idx=-1 if pad is None else pad, eps=1e-5, dropout_p=p, training=1, seed=SEED, offset=offset,
                           d_workspace=bufs["ws"].ptr, workspace_bytes=ws_bytes)
    return a, bufs, ins, want, ref


def test_c_abi_writes_only_its_window():
    """Through ctypes, every output inside NaN-payload guards: the forward writes y, the statistics and (roberta) the positions and
    nothing else -- not the rest of the workspace; the backward writes the workspace, the rows of the tables that occur and the two
    vectors; an output that is not wanted is not written."""
    from ance_amd import _lib
    L_ = _lib.lib()
    st = _lib.current_stream_ptr()
    for mode, pad in (("roberta", 1), ("absolute", None)):
        a, bufs, ins, want, ref = _c_call(mode, pad)
        T_, H = a.n_seq * a.L, a.H
        S = 2 * ((4 * T_ + 255) // 256 * 256)
        _lib.check(L_.ance_embed_forward(ctypes.byref(a), st), "forward")
        torch.cuda.synchronize()
        for name in ("dword", "dpos", "dtype"):
            assert np.all(bufs[name].window() == 0), name
        assert bufs["dgamma"].untouched() and bufs["dbeta"].untouched()
        assert np.all(_bits(bufs["ws"].window())[S // 4:] == NAN32), "the forward writes the statistics only"
        assert bufs["positions"].untouched() == (mode == "absolute")
        if mode == "roberta":
            assert np.array_equal(bufs["positions"].window(), want["positions"].reshape(-1))
        # the grouping, as the wrapper makes it
        sk = {n: torch.sort(t.view(-1), stable=True) for n, t in (("word", ins["ids"]), ("type", ins["types"]), ("pos", bufs["positions"].buf[64:64 + T_]))}
        g = _lib.AnceEmbedGradArgs(dy=ins["dy"].data_ptr(), dword=bufs["dword"].ptr, dpos=bufs["dpos"].ptr, dtype=bufs["dtype"].ptr,
                                   dgamma=bufs["dgamma"].ptr, dbeta=bufs["dbeta"].ptr, word_keys=sk["word"][0].data_ptr(),
                                   word_perm=sk["word"][1].data_ptr(), pos_keys=sk["pos"][0].data_ptr(), pos_perm=sk["pos"][1].data_ptr(),
                                   type_keys=sk["type"][0].data_ptr(), type_perm=sk["type"][1].data_ptr())
        _lib.check(L_.ance_embed_backward(ctypes.byref(a), ctypes.byref(g), st), "backward")
        torch.cuda.synchronize()
        for name, buf in bufs.items():
            assert buf.guards_intact(), name
        rows = want["word_rows"]
        dword = bufs["dword"].window((a.vocab, H))
        rest = np.ones(a.vocab, bool)
        rest[rows] = False
        assert np.all(_bits(dword[rest]) == 0), "rows that do not occur keep the caller's zeros"
        got = dict(y=bufs["y"].window((T_, H)), dword=dword[rows], dpos=bufs["dpos"].window((a.max_pos, H)), dtype=bufs["dtype"].window((2, H)),
                   dgamma=bufs["dgamma"].window(), dbeta=bufs["dbeta"].window())
        _check("C ABI %s" % mode, got, want, ref)
        # every output is optional in the backward
        for k in ("dword", "dpos", "dtype", "dgamma", "dbeta"):
            a2, bufs2, ins2, _, _ = _c_call(mode, pad)
            _lib.check(L_.ance_embed_forward(ctypes.byref(a2), st), "forward")
            g2 = _lib.AnceEmbedGradArgs.from_buffer_copy(g)
            for f in ("dword", "dpos", "dtype", "dgamma", "dbeta"):
                setattr(g2, f, bufs2[f].ptr)
            setattr(g2, k, None)
            _lib.check(L_.ance_embed_backward(ctypes.byref(a2), ctypes.byref(g2), st), "backward")
            torch.cuda.synchronize()
            fresh = _Guarded(bufs2[k].words, fill=0 if k in ("dword", "dpos", "dtype") else None)
            assert torch.equal(bufs2[k].buf, fresh.buf), k
            for o in ("dword", "dpos", "dtype", "dgamma", "dbeta"):
                if o != k:
                    assert np.array_equal(_bits(bufs2[o].window()), _bits(bufs[o].window())), (k, o)


def test_only_wanted_gradients_are_allocated_and_written():
    """requires_grad off on the word table: no dense [vocab, H] tensor is allocated for it -- the peak of forward + backward stays
    below that tensor's size, and lies below the same call's peak with the gradient wanted by at least that size -- no sort of the
    ids and no fill are launched for it, and the other gradients keep their bits.  (leaves[0].grad is None says nothing: autograd
    never assigns a gradient to such a leaf; the memory and the launches do.)"""
    from ance_amd.embeddings import bert_embeddings
    H, vocab = 768, 4000
    dense = 4 * vocab * H   # 12.3 MB; everything else of the call (y, the workspace, the position table's gradient) is about 3 MB
    tables = _tables("wanted", H, vocab, 514, 2)
    ids, types = U.seeded_ids("wanted", (4, 33), 0, vocab), U.seeded_ids("wanted.tt", (4, 33), 0, 2)
    dy = U.embed_dy("wanted", ids.size, H)
    full = _run(ids, types, tables, 1e-5, dy, "roberta", 1)
    tid, ttt, tdy = _dev(ids), _dev(types), _dev(dy).view(4, 33, H)

    def call(word_wanted, trace=False):
        leaves = [_dev(t, word_wanted or i != 0) for i, t in enumerate(tables)]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y = bert_embeddings(tid, *leaves, 1e-5, ttt, "roberta", 1)
        kernels = _traced_kernels(lambda: y.backward(tdy)) if trace else y.backward(tdy)
        torch.cuda.synchronize()
        return leaves, torch.cuda.max_memory_allocated() - base, kernels

    leaves, peak_without, _ = call(False)
    _, peak_with, _ = call(True)
    print("peak of forward + backward above the leaves: %d B without the word gradient, %d B with it; the dense gradient is %d B"
          % (peak_without, peak_with, dense))
    assert leaves[0].grad is None
    assert peak_without < dense, (peak_without, dense)
    assert peak_with - peak_without >= dense, (peak_with, peak_without, dense)
    for n, t in zip(("dpos", "dtype", "dgamma", "dbeta"), leaves[1:]):
        assert np.array_equal(_bits(_np(t.grad)), _bits(full[n])), n
    # the launches: this library's four either way (the position and type tables still need the segmented sum); of torch's, the
    # sort of the ids and whatever fills the dense tensor are gone
    ours = lambda names: [n for n in names if any(k in n for k in KERNELS)]   # noqa: E731
    k_without, k_with = call(False, trace=True)[2], call(True, trace=True)[2]
    print("backward kernels without the word gradient:", k_without)
    print("backward kernels with it:", k_with)
    assert len(ours(k_without)) == len(ours(k_with)) == BACKWARD_LAUNCHES
    assert len(k_without) < len(k_with), (len(k_without), len(k_with))
    for t in leaves:
        t.requires_grad_(False)
    y = bert_embeddings(tid, *leaves, 1e-5, ttt, "roberta", 1)
    assert not y.requires_grad


# ------------------------------------------------------------------------------------------------------------------------ the module
@pytest.mark.parametrize("mode", ["absolute", "roberta"])
def test_module_against_the_expression(mode):
    """BertEmbeddings in training mode, forward + backward, against the util's expression with the restated mask: in fp32 and under
    torch.autocast; then fp16 parameters under autocast are used as fp32 and the output is fp32."""
    from ance_amd import attention as T
    from ance_amd.embeddings import BertEmbeddings
    H, vocab, max_pos, pad, p = 768, 1000, 514, 1, 0.1
    n_types = 2 if mode == "absolute" else 1
    tables = _tables("module", H, vocab, max_pos, n_types)
    ids = U.seeded_ids("module", (3, 50), 0, vocab)
    ids[1, 30:] = pad
    types = U.seeded_ids("module.tt", ids.shape, 0, 2) if n_types == 2 else None
    dy = U.embed_dy("module", ids.size, H)
    m = BertEmbeddings(vocab, H, max_pos, n_types, 1e-5, p, pad_token_id=pad, position_mode=mode).to(DEV)
    m.load_state_dict(dict(zip(U.PARAMS, (torch.from_numpy(t) for t in tables))), strict=True)
    keep, want, ref = _reference(ids, types, tables, 1e-5, dy, mode, pad, p, 0)
    m.train()
    T.manual_seed(SEED)
    y = m(_dev(ids), None if types is None else _dev(types))
    y.backward(_dev(dy).view(y.shape))
    rows = want["word_rows"]
    grads = {U.GRAD_OF[n]: _np(t.grad) for n, t in m.named_parameters()}
    got = dict(grads, y=_np(y).reshape(-1, H), dword=grads["dword"][rows])
    _check("module %s p 0.1" % mode, got, want, ref)
    # the same under torch.autocast (fp32 parameters, as autocast training keeps them): forward and backward go through the
    # autocast wrappers of the Function, the output and the gradients are fp32, held to the same bound -- and are the same bits
    m.zero_grad(set_to_none=True)
    T.manual_seed(SEED)
    with torch.autocast("cuda", dtype=torch.float16):
        y_ac = m(_dev(ids), None if types is None else _dev(types))
        assert y_ac.dtype == torch.float32
        y_ac.backward(_dev(dy).view(y_ac.shape))
    grads_ac = {U.GRAD_OF[n]: _np(t.grad) for n, t in m.named_parameters()}
    assert all(v.dtype == np.float32 for v in grads_ac.values())
    got_ac = dict(grads_ac, y=_np(y_ac).reshape(-1, H), dword=grads_ac["dword"][rows])
    _check("module %s p 0.1 under autocast" % mode, got_ac, want, ref)
    for n in U.NAMES:
        assert np.array_equal(_bits(got_ac[n]), _bits(got[n])), n
    m.eval()
    at = dict(T.dropout_state.offsets)
    y_eval = m(_dev(ids), None if types is None else _dev(types))
    assert T.dropout_state.offsets == at and torch.all(y_eval != 0)
    half = BertEmbeddings(vocab, H, max_pos, n_types, 1e-5, p, pad_token_id=pad, position_mode=mode).to(DEV).half().eval()
    half.load_state_dict(m.state_dict())
    with torch.autocast("cuda", dtype=torch.float16):
        y16 = half(_dev(ids), None if types is None else _dev(types))
    assert y16.dtype == torch.float32
    ref32 = BertEmbeddings(vocab, H, max_pos, n_types, 1e-5, p, pad_token_id=pad, position_mode=mode).to(DEV).eval()
    ref32.load_state_dict({k: v.float() for k, v in half.state_dict().items()})
    assert torch.equal(y16.view(torch.int32), ref32(_dev(ids), None if types is None else _dev(types)).view(torch.int32))
    with pytest.raises(Exception, match="float32"):
        half(_dev(ids))   # outside autocast nothing is cast behind the caller's back
