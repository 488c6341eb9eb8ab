"""Times the assembly of one training batch (msmarco_triplet: query, positive, negative; 9 tensors) from synthetic token caches
generated here -- 1 M passages x 128 tokens, 100 k queries x 64, 2,000 ann_training_data lines x 20 negatives -- in ONE process, the
variants alternated --rounds times (each round times every variant once at every B: --steps batches after --warmup):
  (1) loader   kind "port": the reference's loader restated below (utils/util.py:257-329 EmbeddingCache and StreamingDataset,
               data/msmarco_data.py:275-303 and 337-362, DataLoader(batch_size=B) without workers), then the trainer's
               ``tuple(t.to(device))`` and six ``.long()`` (drivers/run_ann.py:237-254).  A port because the reference's checkout is
               not where the GPU is; host wall time per batch over the window, one synchronise at its end.
  (2) batcher  ance_amd.batches.TrainingBatches(dtype=torch.long) over DeviceTokenCache: host time to enqueue a batch (a window with
               no synchronise inside), device-event time per batch, and the launches per batch traced with torch.profiler.
The yardstick is (1) in the same process on the same box, never an earlier figure of (2).  Writes one JSON object (--out)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_PASSAGES, L_PASSAGE, N_QUERIES, L_QUERY, N_LINES, N_NEG = 1_000_000, 128, 100_000, 64, 2_000, 20


def write_cache(base, n, L, rng, chunk=100_000):
    with open(base, "wb") as f:
        for r0 in range(0, n, chunk):
            m = min(chunk, n - r0)
            lens = rng.integers(1, L + 1, size=m)
            ids = rng.integers(3, 50_000, size=(m, L), dtype=np.int32)
            ids[np.arange(L)[None, :] >= lens[:, None]] = 1
            rec = np.empty((m, 4 + 4 * L), np.uint8)
            rec[:, :4] = lens.astype(">u4").view(np.uint8).reshape(m, 4)
            rec[:, 4:] = ids.astype("<i4").view(np.uint8).reshape(m, 4 * L)
            f.write(rec.tobytes())
    with open(base + "_meta", "w") as f:
        json.dump({"type": "int32", "total_number": n, "embedding_size": L}, f)


# ---- the reference's loader, restated ------------------------------------------------------------------------------------------
class EmbeddingCache:
    """utils/util.py:257-307."""

    def __init__(self, base_path):
        with open(base_path + "_meta") as f:
            meta = json.load(f)
        self.dtype, self.total_number = np.dtype(meta["type"]), meta["total_number"]
        self.record_size = int(meta["embedding_size"]) * self.dtype.itemsize + 4
        self.f = open(base_path, "rb")

    def __getitem__(self, key):
        if key < 0 or key > self.total_number:
            raise IndexError("Index {} is out of bound for cached embeddings of size {}".format(key, self.total_number))
        self.f.seek(key * self.record_size)
        record_bytes = self.f.read(self.record_size)
        return int.from_bytes(record_bytes[:4], "big"), np.frombuffer(record_bytes[4:], dtype=self.dtype)


def processing_fn(max_len, query):
    """data/msmarco_data.py:275-303 (GetProcessingFn)."""
    import torch
    from torch.utils.data import TensorDataset

    def fn(vals, i):
        passage_len, passage = vals
        pad_len = max(0, max_len - passage_len)
        token_type_ids = ([0] if query else [1]) * passage_len + [0] * pad_len
        attention_mask = [1] * passage_len + [0] * pad_len
        passage_collection = [(i, passage, attention_mask, token_type_ids)]
        query2id_tensor = torch.tensor([f[0] for f in passage_collection], dtype=torch.long)
        all_input_ids_a = torch.tensor([f[1] for f in passage_collection], dtype=torch.int)
        all_attention_mask_a = torch.tensor([f[2] for f in passage_collection], dtype=torch.bool)
        all_token_type_ids_a = torch.tensor([f[3] for f in passage_collection], dtype=torch.uint8)
        dataset = TensorDataset(all_input_ids_a, all_attention_mask_a, all_token_type_ids_a, query2id_tensor)
        return [ts for ts in dataset]
    return fn


def triplet_fn(query_cache, passage_cache):
    """data/msmarco_data.py:337-362 (GetTripletTrainingDataProcessingFn)."""
    def fn(line, i):
        line_arr = line.split("\t")
        qid, pos_pid = int(line_arr[0]), int(line_arr[1])
        neg_pids = [int(neg_pid) for neg_pid in line_arr[2].split(",")]
        query_data = processing_fn(L_QUERY, True)(query_cache[qid], qid)[0]
        pos_data = processing_fn(L_PASSAGE, False)(passage_cache[pos_pid], pos_pid)[0]
        for neg_pid in neg_pids:
            neg_data = processing_fn(L_PASSAGE, False)(passage_cache[neg_pid], neg_pid)[0]
            yield (query_data[0], query_data[1], query_data[2], pos_data[0], pos_data[1], pos_data[2],
                   neg_data[0], neg_data[1], neg_data[2])
    return fn


def reference_batches(lines, query_cache, passage_cache, B, device):
    """StreamingDataset (utils/util.py:310-329, one process) under DataLoader(batch_size=B), then drivers/run_ann.py:237-247."""
    from torch.utils.data import DataLoader, IterableDataset

    class StreamingDataset(IterableDataset):
        def __iter__(self):
            fn = triplet_fn(query_cache, passage_cache)
            for i, element in enumerate(lines):
                for rec in fn(element, i):
                    yield rec

    for batch in DataLoader(StreamingDataset(), batch_size=B):
        batch = tuple(t.to(device) for t in batch)
        yield {"query_ids": batch[0].long(), "attention_mask_q": batch[1].long(), "input_ids_a": batch[3].long(),
               "attention_mask_a": batch[4].long(), "input_ids_b": batch[6].long(), "attention_mask_b": batch[7].long()}


# ---- timing ----------------------------------------------------------------------------------------------------------------------
def host_ms_per_batch(it, steps, warmup):
    """Host wall time per batch of a window of `steps` batches, one synchronise at its end (inside the window)."""
    import torch
    keep = [next(it) for _ in range(warmup)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        keep.append(next(it))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def enqueue_ms_per_batch(it, steps, warmup):
    """Host time to enqueue a batch: the window is closed BEFORE the synchronise."""
    import torch
    keep = [next(it) for _ in range(warmup)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        keep.append(next(it))
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) / steps * 1e3


def device_ms_per_batch(it, steps, warmup):
    import torch
    keep = [next(it) for _ in range(warmup)]
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        keep.append(next(it))
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def traced_launches(it, calls):
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    keep = []
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        for _ in range(calls):
            keep.append(next(it))
        torch.cuda.synchronize()
    kernels, copies = {}, 0
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            if "memcpy" in e.name.lower() or "memset" in e.name.lower():
                copies += 1
            else:
                kernels[e.name[:90]] = kernels.get(e.name[:90], 0) + 1
    return dict(kernels_per_batch=round(sum(kernels.values()) / calls, 2), copies_per_batch=round(copies / calls, 2),
                by_name={k: round(v / calls, 2) for k, v in sorted(kernels.items())})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch-sizes", default="8,64,512")
    ap.add_argument("--trace-calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_batches.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_batches.py times the GPU path; there is no CPU measurement"
    from ance_amd.batches import DeviceTokenCache, TrainingBatches
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(10)
    sizes = [int(b) for b in a.batch_sizes.split(",")]
    assert (a.steps + a.warmup + a.trace_calls + 1) * max(sizes) <= N_LINES * N_NEG, "the window needs more items than the lines hold"
    out = dict(what="one msmarco_triplet training batch (9 tensors) from ann_training_data lines and the two token caches",
               device=torch.cuda.get_device_name(0), torch=torch.__version__, rounds=a.rounds, steps=a.steps, warmup=a.warmup,
               inputs=dict(passages=[N_PASSAGES, L_PASSAGE], queries=[N_QUERIES, L_QUERY], lines=N_LINES, negatives_per_line=N_NEG),
               loader=dict(kind="port", of="utils/util.py:257-329, data/msmarco_data.py:275-303 + 337-362, DataLoader(batch_size=B), "
                                          "drivers/run_ann.py:237-247 (.to(device), six .long())",
                           timed="host wall ms per batch, one synchronise at the end of the window"),
               batcher=dict(kind="product", of="ance_amd.batches.TrainingBatches(dtype=torch.long) over DeviceTokenCache"))
    with tempfile.TemporaryDirectory() as tmp:
        qp, pp = os.path.join(tmp, "queries"), os.path.join(tmp, "passages")
        write_cache(qp, N_QUERIES, L_QUERY, rng)
        write_cache(pp, N_PASSAGES, L_PASSAGE, rng)
        lines = ["%d\t%d\t%s\n" % (rng.integers(N_QUERIES), rng.integers(N_PASSAGES),
                                   ",".join(str(x) for x in rng.integers(N_PASSAGES, size=N_NEG))) for _ in range(N_LINES)]
        print("caches written", flush=True)
        t0 = time.perf_counter()
        dq, dp = DeviceTokenCache(qp, dev), DeviceTokenCache(pp, dev)
        torch.cuda.synchronize()
        out["batcher"]["cache_upload_s"] = round(time.perf_counter() - t0, 3)
        out["batcher"]["cache_bytes_on_device"] = dict(queries=dq.records.numel(), passages=dp.records.numel())
        hq, hp = EmbeddingCache(qp), EmbeddingCache(pp)
        t0 = time.perf_counter()
        TrainingBatches(lines, dq, dp, 8, "msmarco_triplet", L_QUERY, L_PASSAGE, dtype=torch.long)
        out["batcher"]["plan_s"] = round(time.perf_counter() - t0, 4)

        # the two variants give the same tensors (first batches at the smallest B)
        ref_it = reference_batches(lines, hq, hp, sizes[0], dev)
        our_it = iter(TrainingBatches(lines, dq, dp, sizes[0], "msmarco_triplet", L_QUERY, L_PASSAGE, dtype=torch.long))
        for _ in range(3):
            r, o = next(ref_it), next(our_it)
            for k, i in (("query_ids", 0), ("attention_mask_q", 1), ("input_ids_a", 3), ("attention_mask_a", 4),
                         ("input_ids_b", 6), ("attention_mask_b", 7)):
                assert r[k].dtype == o[i].dtype and torch.equal(r[k], o[i]), k
        out["variants_agree"] = True

        res = {}
        for B in sizes:
            seen = dict(loader_host_ms=[], batcher_host_enqueue_ms=[], batcher_device_ms=[], batcher_host_ms=[])
            for _ in range(a.rounds):
                seen["loader_host_ms"].append(host_ms_per_batch(reference_batches(lines, hq, hp, B, dev), a.steps, a.warmup))
                mk = lambda: iter(TrainingBatches(lines, dq, dp, B, "msmarco_triplet", L_QUERY, L_PASSAGE, dtype=torch.long))  # noqa: E731
                seen["batcher_host_ms"].append(host_ms_per_batch(mk(), a.steps, a.warmup))
                seen["batcher_host_enqueue_ms"].append(enqueue_ms_per_batch(mk(), a.steps, a.warmup))
                seen["batcher_device_ms"].append(device_ms_per_batch(mk(), a.steps, a.warmup))
                print("B", B, "round", {k: round(v[-1], 4) for k, v in seen.items()}, flush=True)
            r = {k: dict(median=round(statistics.median(v), 4), rounds=[round(x, 4) for x in v]) for k, v in seen.items()}
            # like for like: host wall time per batch with one synchronise at the end of the window, both variants
            r["loader_over_batcher"] = round(r["loader_host_ms"]["median"] / r["batcher_host_ms"]["median"], 1)
            r["batcher_faster_in_every_round"] = max(seen["batcher_host_ms"]) < min(seen["loader_host_ms"])
            if a.trace_calls > 0:
                try:
                    it = mk()
                    next(it)   # the plan's upload belongs to the pass, not to a batch
                    r["batcher_traced"] = traced_launches(it, a.trace_calls)
                except Exception as e:  # pragma: no cover - depends on the profiler of the torch build
                    r["batcher_traced"] = dict(unavailable=repr(e))
            res["B=%d" % B] = r
        out["results"] = res
    print(json.dumps(out), flush=True)
    if a.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
