"""ance_amd.batches on the GPU: every batch TrainingBatches yields equals the slice of the item stream the reference's real loaders
produced (tests/golden/batches.npz; generator: tests/golden/make_golden_batches.py, fixture: tests/batches_util.py), in every tuple
position, in the reference's dtypes and in the wide form.  All comparisons are exact.  The index clamp of the kernel is not
exercised here (an index outside the records never reaches it: the plan refuses it); it is one line of csrc/batch_gather.hip."""
import json
import os
import random

import numpy as np
import pytest

import batches_util as U
from ance_amd import _lib
from ance_amd.cache import TokenCache

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "batches.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(golden_dir, "batches.npz")), meta


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    from ance_amd.batches import DeviceTokenCache
    d = str(tmp_path_factory.mktemp("batches"))
    out = {}
    for case in U.CASES:
        qp, pp, lines = U.build_case(case, d)
        out[case] = (DeviceTokenCache(qp, "cuda:0"), DeviceTokenCache(pp, "cuda:0"), lines)
    return out


def make(cases, case, form, world=1, rank=0, batch_size=4, dtype=None):
    from ance_amd.batches import TrainingBatches
    qc, pc, lines = cases[case]
    c = U.CASES[case]
    return TrainingBatches(lines, qc, pc, batch_size, form, c["L_q"], c["L_p"], rank=rank, world_size=world, dtype=dtype)


def widened(x, position, wide):
    """The golden array of a tuple position as the wide form has it: ids and masks int64, token types and labels as they are."""
    return x.astype(np.int64) if wide and position < 9 and position % 3 != 2 else x


def check_pass(tb, stream, wide):
    """Every batch of one pass against the consecutive slices of ``stream`` (a list of arrays per tuple position)."""
    import torch
    batches = list(tb)
    torch.cuda.synchronize()
    n, B = len(stream[0]), tb.batch_size
    assert len(batches) == len(tb) == -(-n // B)
    for k, batch in enumerate(batches):
        assert len(batch) == len(stream)
        for i, t in enumerate(batch):
            want = widened(stream[i][k * B:(k + 1) * B], i, wide)
            assert t.is_cuda and t.is_contiguous() and tuple(t.shape) == want.shape, (k, i, t.shape, want.shape)
            got = t.cpu().numpy()
            assert got.dtype == want.dtype and np.array_equal(got, want), (k, i)


def test_device_cache_is_the_file(cases, tmp_path):
    import torch
    from ance_amd.batches import DeviceTokenCache
    qc, pc, _ = cases["small"]
    host = TokenCache(pc.base_path)
    assert len(pc) == len(host) == 37 and pc.embedding_size == host.embedding_size == 20
    assert pc.records.dtype == torch.uint8 and tuple(pc.records.shape) == (37, 84)
    assert np.array_equal(pc.records.cpu().numpy(), np.asarray(host.records()))
    with DeviceTokenCache(qc.base_path) as c:                 # the context-manager protocol; the default device
        assert len(c) == 11 and c.records.is_cuda
    lens, ids = U.cache_arrays(0, 8, 1, 1)
    U.write_cache(str(tmp_path / "empty"), lens, ids)
    assert tuple(DeviceTokenCache(str(tmp_path / "empty")).records.shape) == (0, 36)


@pytest.mark.parametrize("case,form,world,rank", U.combos())
def test_batches_equal_the_reference_loader(golden, cases, case, form, world, rank):
    import torch
    arrays, meta = golden
    key = U.key(case, form, world, rank)
    stream = [arrays["%s.%d" % (key, i)] for i in range(meta["combos"][key]["arity"])]
    for B in U.BATCH_SIZES:
        for dtype in (None, torch.long):
            random.seed(U.DPR_SEED)
            check_pass(make(cases, case, form, world, rank, B, dtype), stream, dtype is torch.long)


@pytest.mark.parametrize("form", U.MSMARCO_FORMS)
def test_two_passes_are_identical(golden, cases, form):
    arrays, meta = golden
    key = U.key("real", form, 1, 0)
    stream = [arrays["%s.%d" % (key, i)] for i in range(meta["combos"][key]["arity"])]
    tb = make(cases, "real", form, batch_size=5)
    check_pass(tb, stream, False)
    check_pass(tb, stream, False)


@pytest.mark.parametrize("form", U.DPR_FORMS)
@pytest.mark.parametrize("world,rank", ((1, 0), (3, 2)))
def test_dpr_second_pass_draws_again(golden, cases, form, world, rank):
    arrays, meta = golden
    key = U.key("dpr", form, world, rank)
    n = meta["combos"][key]["arity"]
    random.seed(U.DPR_SEED)
    tb = make(cases, "dpr", form, world, rank, batch_size=5)
    check_pass(tb, [arrays["%s.%d" % (key, i)] for i in range(n)], False)
    check_pass(tb, [arrays["%s.pass2.%d" % (key, i)] for i in range(n)], False)


def test_gather_on_a_side_stream_with_its_consumer(golden, cases):
    """The gather goes to the current stream: a consumer enqueued behind it on the same side stream reads finished batches with no
    synchronisation in between."""
    import torch
    arrays, meta = golden
    key = U.key("maxp", "msmarco_triplet", 1, 0)
    stream = [arrays["%s.%d" % (key, i)] for i in range(9)]
    side = torch.cuda.Stream()
    sums = []
    with torch.cuda.stream(side):
        for batch in make(cases, "maxp", "msmarco_triplet", batch_size=5, dtype=torch.long):
            sums.append(torch.stack([batch[i].sum() for i in (0, 1, 3, 4, 6, 7)]))
        got = torch.stack(sums)
    side.synchronize()
    want = [[int(stream[i][k:k + 5].astype(np.int64).sum()) for i in (0, 1, 3, 4, 6, 7)] for k in range(0, len(stream[0]), 5)]
    assert got.cpu().tolist() == want


@pytest.mark.parametrize("wide", (False, True))
@pytest.mark.parametrize("misalign", (False, True))
def test_every_output_byte_is_written_and_none_outside(tmp_path, wide, misalign):
    """ance_gather_batch called directly on poison-filled raw buffers: L = 7 and B = 3 (21 tokens: rows straddle a thread's four
    tokens and the last token stands alone) and L = 20, B = 5; outputs 16-byte aligned and at the smallest alignment the call
    accepts.  Two different poisons give the same, expected bytes -- so no poison byte survives -- and the guard bytes on both
    sides of every output keep theirs."""
    import torch
    from ance_amd.batches import DeviceTokenCache
    L = _lib.lib()
    GUARD = 64
    for n_rec, Lr, B, first, seed in ((5, 7, 3, 1, 91), (37, 20, 5, 2, 92)):
        lens, ids = U.cache_arrays(n_rec, Lr, 1, seed)
        base = str(tmp_path / ("c%d_%d_%d" % (Lr, wide, misalign)))
        U.write_cache(base, lens, ids)
        cache, host = DeviceTokenCache(base, "cuda:0"), TokenCache(base)
        index = np.array([(3 * i + 1) % n_rec for i in range(first + B)], np.int64)
        d_index = torch.from_numpy(index).cuda()
        want_ids, want_mask, want_types = U.numpy_gather(host, index[first:], False, True)
        if wide:
            want_ids, want_mask = want_ids.astype(np.int64), want_mask.astype(np.int64)
        want = [np.ascontiguousarray(w).view(np.uint8).reshape(-1) for w in (want_ids, want_mask, want_types)]
        shift = ((8 if wide else 4), (8 if wide else 4), 4) if misalign else (0, 0, 0)
        for poison in (0xA5, 0x5A):
            bufs = [torch.full((GUARD + sh + len(w) + GUARD,), poison, dtype=torch.uint8, device="cuda:0") for w, sh in zip(want, shift)]
            assert all(b.data_ptr() % 16 == 0 for b in bufs)
            seg = (_lib.AnceGatherSegment * 1)()
            s = seg[0]
            s.d_records, s.n_records, s.d_index, s.n_index, s.L = cache.records.data_ptr(), n_rec, d_index.data_ptr(), len(index), Lr
            s.mask_rule, s.type_rule = _lib.GATHER_MASK_LENGTH, _lib.GATHER_TYPES_LENGTH
            s.d_ids, s.d_mask, s.d_types = (b.data_ptr() + GUARD + sh for b, sh in zip(bufs, shift))
            rc = L.ance_gather_batch(seg, 1, first, B, _lib.GATHER_WIDE if wide else _lib.GATHER_REFERENCE, _lib.current_stream_ptr())
            assert rc == 0, L.ance_last_error()
            torch.cuda.synchronize()
            got = [b.cpu().numpy() for b in bufs]
            for g, w, sh in zip(got, want, shift):
                assert (g[:GUARD + sh] == poison).all() and (g[GUARD + sh + len(w):] == poison).all()
                assert np.array_equal(g[GUARD + sh:GUARD + sh + len(w)], w)
        # without token types: the other two outputs as before, nothing else touched
        bufs = [torch.full((GUARD + len(w) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0") for w in want[:2]]
        s.d_ids, s.d_mask, s.d_types = bufs[0].data_ptr() + GUARD, bufs[1].data_ptr() + GUARD, None
        assert L.ance_gather_batch(seg, 1, first, B, _lib.GATHER_WIDE if wide else _lib.GATHER_REFERENCE, _lib.current_stream_ptr()) == 0
        torch.cuda.synchronize()
        for b, w in zip(bufs, want[:2]):
            g = b.cpu().numpy()
            assert np.array_equal(g[GUARD:GUARD + len(w)], w) and (g[:GUARD] == 0xA5).all() and (g[GUARD + len(w):] == 0xA5).all()
