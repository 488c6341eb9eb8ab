"""Generates tests/golden/batches.npz and batches.json (CPU; needs the reference checkout, oracle/ref_harness.py):

    python tests/golden/make_golden_batches.py

Runs the reference's REAL loaders -- utils/util.py EmbeddingCache and StreamingDataset, data/msmarco_data.py and data/DPR_data.py
Get(Triplet)TrainingDataProcessingFn, torch.utils.data.DataLoader -- on the caches and lines of tests/batches_util.py, for every
(case, form, world, rank) of batches_util.combos().  Stored per combination: the concatenated item stream, one array per tuple
position (``<key>.<position>``), and the record indices the loader read for it (``<key>.plan.q|a|b``: taken from the keys its two
caches were asked for, in order).  This script itself asserts, for batch sizes 1, 4, 5 and 64, that the reference's batches are the
consecutive slices of that stream -- so the tests may slice.

The rank striding of StreamingDataset reads torch.distributed; a stand-in with the three functions it calls replaces
``utils.util.dist`` for the run.  The DPR forms shuffle with Python's global ``random``: every pass starts from
``random.seed(batches_util.DPR_SEED)``; batches.json records the generator state after one pass, and a SECOND pass that goes on from
there is stored as ``<key>.pass2.*``.
"""
import importlib
import json
import os
import random
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import batches_util as U  # noqa: E402
from oracle import ref_harness  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
CHECKED_BATCH_SIZES = (1, 4, 5, 64)


class Recording:
    """An EmbeddingCache that notes the keys it is asked for."""

    def __init__(self, cache):
        self.cache, self.keys = cache, []

    def __getitem__(self, k):
        self.keys.append(int(k))
        return self.cache[k]


def loader_fn(ref, dpr_data, form, args, qc, pc):
    mod = dpr_data if form.startswith("dpr") else ref.msmarco_data
    make = mod.GetTripletTrainingDataProcessingFn if form.endswith("triplet") else mod.GetTrainingDataProcessingFn
    return make(args, qc, pc)


def one_pass(ref, dpr_data, form, args, qc, pc, lines, batch_size):
    """(batches as lists of arrays, query keys, passage keys) of one pass of the reference's loader."""
    from torch.utils.data import DataLoader
    q, p = Recording(qc), Recording(pc)
    ds = ref.util.StreamingDataset(lines, loader_fn(ref, dpr_data, form, args, q, p))
    batches = [[t.numpy() for t in b] for b in DataLoader(ds, batch_size=batch_size)]
    return batches, q.keys, p.keys


def plan_from_keys(form, n_neg, qk, pk):
    """The (q, a, b) record indices of every item, from the keys the loader asked its caches for.  Per kept line the MS MARCO
    loaders read the query, the positive and every negative; the DPR loaders the query, the positive and the chosen negative."""
    q, a, b = [], [], []
    pi = 0
    for line, k in enumerate(n_neg):
        if form.startswith("dpr"):
            k = 1
        pos, negs = pk[pi], pk[pi + 1:pi + 1 + k]
        pi += 1 + k
        for neg in negs:
            if form.endswith("triplet"):
                q.append(qk[line])
                a.append(pos)
                b.append(neg)
            else:
                q += [qk[line]] * 2
                a += [pos, neg]
                b += [-1, -1]
    assert pi == len(pk) and len(qk) == len(n_neg)
    return dict(q=np.array(q, np.int64), a=np.array(a, np.int64), b=np.array(b, np.int64))


def main():
    ref = ref_harness.load_reference()
    dpr_data = importlib.import_module("data.DPR_data")
    arrays, meta = {}, dict(generator="tests/golden/make_golden_batches.py", dpr_seed=U.DPR_SEED,
                            checked_batch_sizes=list(CHECKED_BATCH_SIZES), combos={}, random_state_after_one_pass={})
    real_dist = ref.util.dist
    with tempfile.TemporaryDirectory() as tmp:
        for case in U.CASES:
            qp, pp, lines = U.build_case(case, tmp)
            c = U.CASES[case]
            args = types.SimpleNamespace(max_query_length=c["L_q"], max_seq_length=c["L_p"])
            for form in U.forms_of(case):
                for world, rank in U.WORLDS:
                    ref.util.dist = types.SimpleNamespace(is_initialized=lambda: True, get_world_size=lambda w=world: w,
                                                          get_rank=lambda r=rank: r)
                    key = U.key(case, form, world, rank)
                    n_neg = [ln.count(",") + 1 for ln in lines[rank::world]]
                    with ref.util.EmbeddingCache(qp) as qc, ref.util.EmbeddingCache(pp) as pc:
                        streams = {}
                        for B in CHECKED_BATCH_SIZES:
                            random.seed(U.DPR_SEED)
                            batches, qk, pk = one_pass(ref, dpr_data, form, args, qc, pc, lines, B)
                            streams[B] = [np.concatenate([b[i] for b in batches]) for i in range(len(batches[0]))]
                            sizes = [len(b[0]) for b in batches]
                            n = sum(sizes)
                            assert sizes == [B] * (n // B) + ([n % B] if n % B else []), (key, B, sizes)
                            if B == CHECKED_BATCH_SIZES[0]:
                                plan, state = plan_from_keys(form, n_neg, qk, pk), random.getstate()
                                if form.startswith("dpr"):   # the second pass goes on from the first one's state
                                    batches2, qk2, pk2 = one_pass(ref, dpr_data, form, args, qc, pc, lines, B)
                                    plan2 = plan_from_keys(form, n_neg, qk2, pk2)
                                    stream2 = [np.concatenate([b[i] for b in batches2]) for i in range(len(batches2[0]))]
                        first = streams[CHECKED_BATCH_SIZES[0]]
                        for B in CHECKED_BATCH_SIZES[1:]:   # the batches are the consecutive B-slices of one stream
                            assert len(streams[B]) == len(first)
                            for x, y in zip(first, streams[B]):
                                assert x.dtype == y.dtype and np.array_equal(x, y), (key, B)
                    for i, x in enumerate(first):
                        arrays["%s.%d" % (key, i)] = x
                    for k, v in plan.items():
                        arrays["%s.plan.%s" % (key, k)] = v
                    meta["combos"][key] = dict(items=int(len(first[0])), arity=len(first),
                                               dtypes=[str(x.dtype) for x in first], shapes=[list(x.shape[1:]) for x in first])
                    if form.startswith("dpr"):
                        for i, x in enumerate(stream2):
                            arrays["%s.pass2.%d" % (key, i)] = x
                        for k, v in plan2.items():
                            arrays["%s.pass2.plan.%s" % (key, k)] = v
                        meta["random_state_after_one_pass"][key] = [state[0], list(state[1]), state[2]]
    ref.util.dist = real_dist
    np.savez_compressed(os.path.join(OUT, "batches.npz"), **arrays)
    with open(os.path.join(OUT, "batches.json"), "w") as f:
        json.dump(meta, f, sort_keys=True)
    print("batches.npz %d B, batches.json %d B; %d combinations" % (
        os.path.getsize(os.path.join(OUT, "batches.npz")), os.path.getsize(os.path.join(OUT, "batches.json")), len(meta["combos"])))
    for k in ("dpr.dpr_triplet.w1r0", "dpr.dpr_pair.w1r0", "small.msmarco_triplet.w1r0", "small.msmarco_pair.w1r0"):
        print(k, meta["combos"][k])


if __name__ == "__main__":
    main()
