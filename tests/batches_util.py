"""The fixture of the training-batch tests (tests/test_batches.py, tests/test_gpu_batches.py) and of the generator of their goldens
(tests/golden/make_golden_batches.py): small token caches in the reference's file format, the ann_training_data lines that read
them, and a NumPy restatement of the gather.  Everything comes from the integer generator below, not from a library's random stream,
so the generator script and the tests build the same bytes.

Cases -- the smallest shapes at which the gather can still be wrong:
  small  passages 37 x 20 (row stride 84 bytes: rows are not 16-byte aligned), queries 11 x 8, pad id 1
  real   passages 9 x 128 (stride 516), queries 5 x 64
  maxp   passages 3 x 2048 (a row is longer than a workgroup's tokens), queries 5 x 64
  dpr    passages 23 x 24, queries 7 x 24 (equal lengths, as data/DPR_data.py writes them), pad id 0; passage 4 has a 0 token before
         its last non-zero token, so its mask follows the ids and not the length
Record lengths include 0, 1, L - 1 and L in every cache that has four records.  Nine lines with 1 to 4 negatives; they include
repeated pids, record 0 and record N - 1 of both caches.

The MS MARCO forms run on every case.  The DPR forms run on ``dpr`` alone: data/DPR_data.py reads both caches with one
max_seq_length, and TrainingBatches refuses caches whose embedding_size differs from it.
"""
import json
import os

import numpy as np

CASES = {
    "small": dict(n_p=37, L_p=20, n_q=11, L_q=8, pad=1),
    "real": dict(n_p=9, L_p=128, n_q=5, L_q=64, pad=1),
    "maxp": dict(n_p=3, L_p=2048, n_q=5, L_q=64, pad=1),
    "dpr": dict(n_p=23, L_p=24, n_q=7, L_q=24, pad=0),
}
MSMARCO_FORMS = ("msmarco_triplet", "msmarco_pair")
DPR_FORMS = ("dpr_triplet", "dpr_pair")
WORLDS = ((1, 0), (2, 0), (2, 1), (3, 2))
BATCH_SIZES = (1, 5, 64)
N_LINES = 9
DPR_SEED = 20240607
ARITY = {"msmarco_triplet": 9, "msmarco_pair": 7, "dpr_triplet": 9, "dpr_pair": 6}


def forms_of(case):
    return MSMARCO_FORMS + (DPR_FORMS if case == "dpr" else ())


def combos():
    return [(c, f, w, r) for c in CASES for f in forms_of(c) for (w, r) in WORLDS]


def key(case, form, world, rank):
    return "%s.%s.w%dr%d" % (case, form, world, rank)


class Lcg:
    """x <- (1103515245 x + 12345) mod 2^31; the draw is bits 16 and up."""

    def __init__(self, seed):
        self.x = seed & 0x7FFFFFFF

    def below(self, n):
        self.x = (1103515245 * self.x + 12345) & 0x7FFFFFFF
        return (self.x >> 16) % n


def record_lengths(n, L, g):
    fixed = [0, 1, L - 1, L] if n >= 4 else [L, 1, L // 2][:n]
    return [fixed[i] if i < len(fixed) else g.below(L + 1) for i in range(n)]


def cache_arrays(n, L, pad, seed):
    """(lengths [n], ids int32 [n, L]): ids in [2, 30000) below the length, the pad id after it."""
    g = Lcg(seed)
    lens = record_lengths(n, L, g)
    ids = np.full((n, L), pad, np.int32)
    for i, ln in enumerate(lens):
        for t in range(ln):
            ids[i, t] = 2 + g.below(29998)
    return np.array(lens, np.int64), ids


def write_cache(base_path, lens, ids):
    n, L = ids.shape
    with open(base_path, "wb") as f:
        for i in range(n):
            f.write(int(lens[i]).to_bytes(4, "big") + ids[i].astype("<i4").tobytes())
    with open(base_path + "_meta", "w") as f:
        json.dump({"type": "int32", "total_number": n, "embedding_size": L}, f)


def lines_of(case):
    """Nine ``qid \\t pos \\t negs`` lines: line i has 1 + i % 4 negatives."""
    c = CASES[case]
    g = Lcg(977 + len(case))
    lines = []
    for i in range(N_LINES):
        q = (0, c["n_q"] - 1)[i] if i < 2 else g.below(c["n_q"])
        pos = (c["n_p"] - 1, 0)[i] if i < 2 else g.below(c["n_p"])
        negs = [g.below(c["n_p"]) for _ in range(1 + i % 4)]
        if i == 3:
            negs[1] = negs[0]                 # a repeated pid within a line
        if i == 5:
            negs[0], negs[1] = 0, c["n_p"] - 1
        if i == 6:
            negs[0] = pos                     # the positive among its negatives
        lines.append("%d\t%d\t%s\n" % (q, pos, ",".join(str(x) for x in negs)))
    return lines


def build_case(case, directory):
    """Writes the two caches of ``case`` under ``directory``; returns (query base path, passage base path, lines)."""
    c = CASES[case]
    os.makedirs(directory, exist_ok=True)
    qp, pp = os.path.join(directory, case + "_queries"), os.path.join(directory, case + "_passages")
    write_cache(qp, *cache_arrays(c["n_q"], c["L_q"], c["pad"], 11 + len(case)))
    lens, ids = cache_arrays(c["n_p"], c["L_p"], c["pad"], 23 + len(case))
    if case == "dpr":                         # passage 4: ten tokens, the fourth of them 0
        lens[4] = 10
        ids[4] = c["pad"]
        ids[4, :10] = [101, 2054, 2003, 0, 1996, 3007, 1997, 2605, 1029, 102]
    write_cache(pp, lens, ids)
    return qp, pp, lines_of(case)


def numpy_gather(cache, index, dpr, passage):
    """(ids int32, mask bool, types uint8), each [n, L]: the rows ``index`` of a TokenCache under a form's rules
    (data/msmarco_data.py:280-282: mask 1 x len, types 1 x len for a passage and 0 for a query; data/DPR_data.py:282-283:
    mask ids != 0, types 0)."""
    index = np.asarray(index, np.int64)
    ids = cache.ids()[index]
    lens = cache.lengths()[index].astype(np.int64)
    in_len = np.arange(cache.embedding_size)[None, :] < lens[:, None]
    if dpr:
        return ids, ids != 0, np.zeros(ids.shape, np.uint8)
    return ids, in_len, (in_len if passage else np.zeros_like(in_len)).astype(np.uint8)


def expected_stream(form, plan, query_cache, passage_cache):
    """The whole item stream of a plan as a list of arrays in the loader's tuple positions."""
    dpr = form.startswith("dpr")
    out = list(numpy_gather(query_cache, plan["q"], dpr, False)) + list(numpy_gather(passage_cache, plan["a"], dpr, True))
    if form.endswith("triplet"):
        out += list(numpy_gather(passage_cache, plan["b"], dpr, True))
    if form == "msmarco_pair":
        out.append(plan["label"])
    return out
