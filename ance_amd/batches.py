"""The trainers' batches, assembled on the GPU from ``ann_training_data_N`` and the two token caches.

The reference builds them in one Python process, serial with the step (``DataLoader(..., batch_size=B)`` without workers over a
``StreamingDataset``: drivers/run_ann.py:199-208, drivers/run_ann_dpr.py:150-157): per item three ``seek`` + ``read`` calls on the
cache files (utils/util.py:292-298) and twelve ``torch.tensor(list_of_arrays)`` constructions (data/msmarco_data.py:275-362,
data/DPR_data.py:276-344), per batch default collation, nine host-to-device copies and six ``.long()`` casts
(drivers/run_ann.py:237-254).

Here the cache files are resident in HBM as their own bytes (``DeviceTokenCache``), the item list of the whole file (the *plan*:
which query, first passage and second passage every item reads) is parsed once and uploaded once, and a batch is ONE launch of
``ance_gather_batch`` (csrc/batch_gather.hip) on the current stream: no host-to-device copy, no synchronisation, no Python per item.
"""
import json
import random

import numpy as np

from . import _lib

FORMS = ("msmarco_triplet", "msmarco_pair", "dpr_triplet", "dpr_pair")
UPLOAD_CHUNK_BYTES = 64 << 20


class DeviceTokenCache:
    """A token cache file (``TokenCache``'s format and ``_meta`` handling) uploaded once: ``.records`` is the file's bytes as a CUDA
    uint8 tensor [N, 4 + 4 L].  Memory: N (4 + 4 L) bytes -- 4.56 GB for the 8.8 M MS MARCO passages at L = 128, 26 GB for the MaxP
    document cache at 4 x 512."""

    def __init__(self, base_path, device=None):
        import torch
        self.base_path = base_path
        with open(base_path + "_meta", "r") as f:
            meta = json.load(f)
        self.dtype = np.dtype(meta["type"])
        if self.dtype != np.dtype("int32"):
            raise ValueError("unsupported cache dtype %s" % self.dtype)
        self.total_number = int(meta["total_number"])
        self.embedding_size = int(meta["embedding_size"])
        self.record_size = self.embedding_size * self.dtype.itemsize + 4
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.records = torch.empty((self.total_number, self.record_size), dtype=torch.uint8, device=self.device)
        if self.total_number:
            mm = np.memmap(base_path, dtype=np.uint8, mode="r", shape=(self.total_number, self.record_size))
            rows = max(1, UPLOAD_CHUNK_BYTES // self.record_size)
            for r0 in range(0, self.total_number, rows):
                self.records[r0:r0 + rows].copy_(torch.from_numpy(np.array(mm[r0:r0 + rows])))
            del mm

    # context-manager protocol kept for call-shape parity with EmbeddingCache
    def open(self):
        return self

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def __len__(self):
        return self.total_number


def parse_lines(lines):
    """``qid \\t pos_pid \\t neg,neg,...`` lines -> (qid [n], pos_pid [n], negatives (flat), negatives per line [n]), all int64.
    One ``split`` of the whole text and array arithmetic on its bytes: no Python per line or per id."""
    text = "\n".join(line.rstrip("\r\n") for line in lines)
    n = len(lines)
    if n == 0:
        z = np.zeros(0, np.int64)
        return z, z, z, z
    raw = np.frombuffer(text.encode("ascii"), dtype=np.uint8)
    line_of = np.cumsum(raw == 10)                     # the line a byte belongs to (a newline counts to the line it opens)
    tabs = np.bincount(line_of[raw == 9], minlength=n)
    if (tabs != 2).any():
        raise ValueError("line %d is not 'qid \\t pos_pid \\t neg,neg,...'" % int(np.flatnonzero(tabs != 2)[0]))
    n_neg = np.bincount(line_of[raw == 44], minlength=n).astype(np.int64) + 1
    tokens = text.replace("\t", " ").replace(",", " ").split()
    if len(tokens) != int(n_neg.sum()) + 2 * n:
        raise ValueError("an empty field in the training lines")
    vals = np.array(tokens).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(n_neg + 2)[:-1]])
    is_neg = np.ones(len(vals), bool)
    is_neg[start] = False
    is_neg[start + 1] = False
    return vals[start], vals[start + 1], vals[is_neg], n_neg


class TrainingBatches:
    """Iterable over the batches one of the reference's four loaders yields, item for item, as tuples of CUDA tensors.

    ``lines``: a list of strings or the path of an ``ann_training_data_N`` file.  ``form``:
      msmarco_triplet  data/msmarco_data.py:337-362: one item per negative, (q, pos, neg): 9 tensors
      msmarco_pair     data/msmarco_data.py:306-334: two items per negative, (q, pos, label 1) then (q, neg, label 0): 7 tensors
      dpr_triplet      data/DPR_data.py:323-344: one item per line, (q, pos, the first negative after random.shuffle): 9 tensors
      dpr_pair         data/DPR_data.py:299-320: two items per line, (q, pos) then (q, neg): 6 tensors, no label
    Every tower contributes (ids, mask, token types), so the token types sit at positions 2, 5 and 8; labels are int64 [B].
    ids are int32, masks bool and types uint8 as the reference's; ``dtype=torch.long`` makes ids and masks int64, which is what the
    trainers' ``.long()`` produces, so they can drop the casts (types stay uint8).

    Lines are strided over ranks as ``StreamingDataset`` does (utils/util.py:318-329): line i is kept when
    ``i % world_size == rank``; a skipped line draws nothing from ``random``.  Batches are consecutive slices of the item stream:
    they cross line boundaries and the last one may be short (``DataLoader``'s default).  ``len()`` is the number of batches.

    The plan (``.plan``: host int64 arrays ``q, a, b, label``, one entry per item, -1 where the form has none) is made when the
    object is, and every id in it is checked then: an id outside [0, N) raises ``IndexError`` with the reference's message.  The
    reference's ``EmbeddingCache`` tolerates ``key == N`` and fails later, in ``stack``, on the short read; here N is refused like
    any other.  The DPR forms check every negative of a kept line, not only the one the shuffle will choose.  A ``max_query_length``
    or ``max_seq_length`` that differs from its cache's ``embedding_size`` raises ``ValueError`` (the reference fails in
    ``default_collate``); the DPR loaders use ``max_seq_length`` for both towers, so ``max_query_length`` is not looked at there.
    A header length above L counts as L, as ``TokenCache.lengths`` has it.

    The DPR forms call ``random.shuffle`` on Python's global ``random`` once per kept line, in line order, with a list as long as
    the line's negatives -- the reference's draws.  They are drawn at each ``iter()`` for the WHOLE pass (``draw_pass``), and a
    second pass draws again, as re-iterating the reference's dataset does.  The reference's loader is lazy: it draws a line's
    shuffle when the batch that holds the line is built.  A caller who draws from ``random`` between batches therefore sees a
    different interleaving here; one who does not sees the same stream.

    Iteration needs ``DeviceTokenCache`` caches; the plan alone (``.plan``, ``draw_pass``) works with ``TokenCache`` and no GPU.
    Each batch costs one ``ance_gather_batch`` call on the current stream and fresh ``torch.empty`` outputs.  Labels are slices of
    the uploaded plan: treat them as read-only.
    """

    def __init__(self, lines, query_cache, passage_cache, batch_size, form, max_query_length, max_seq_length, rank=0,
                 world_size=1, dtype=None):
        if form not in FORMS:
            raise ValueError("unknown form %r: one of %s" % (form, ", ".join(FORMS)))
        if batch_size < 1:
            raise ValueError("batch_size %r < 1" % (batch_size,))
        if world_size < 1 or not 0 <= rank < world_size:
            raise ValueError("rank %r outside [0, world_size = %r)" % (rank, world_size))
        self.form, self.batch_size = form, int(batch_size)
        self.dpr, self.triplet = form.startswith("dpr"), form.endswith("triplet")
        self.query_cache, self.passage_cache = query_cache, passage_cache
        want_q = max_seq_length if self.dpr else max_query_length
        for what, want, cache in (("max_seq_length" if self.dpr else "max_query_length", want_q, query_cache),
                                  ("max_seq_length", max_seq_length, passage_cache)):
            if int(want) != cache.embedding_size:
                raise ValueError("%s = %d, but the cache %s holds records of embedding_size %d" % (
                    what, want, cache.base_path, cache.embedding_size))
        self.wide = False
        if dtype is not None:
            import torch
            if dtype not in (torch.long, torch.int32):
                raise ValueError("dtype %r: torch.long (wide) or None / torch.int32 (the reference's dtypes)" % (dtype,))
            self.wide = dtype == torch.long
        if isinstance(lines, str):
            with open(lines, "r") as f:
                lines = f.readlines()
        lines = list(lines)[rank::world_size]
        qid, pos, neg, n_neg = parse_lines(lines)
        self._check_ids(qid, pos, neg, n_neg)
        self._qid, self._pos, self._neg, self._n_neg = qid, pos, neg, n_neg
        self._neg_start = np.concatenate([[0], np.cumsum(n_neg)[:-1]]).astype(np.int64) if len(n_neg) else n_neg
        none = lambda n: np.full(n, -1, np.int64)  # noqa: E731
        if self.dpr:
            n = len(qid) * (1 if self.triplet else 2)
            self.n_items = n
            self.plan = None  # made by draw_pass
        elif self.triplet:
            q, a = np.repeat(qid, n_neg), np.repeat(pos, n_neg)
            self.n_items = len(q)
            self.plan = dict(q=q, a=a, b=neg.copy(), label=none(len(q)))
        else:
            q = np.repeat(qid, 2 * n_neg)
            a = np.empty(len(q), np.int64)
            a[0::2], a[1::2] = np.repeat(pos, n_neg), neg
            label = np.zeros(len(q), np.int64)
            label[0::2] = 1
            self.n_items = len(q)
            self.plan = dict(q=q, a=a, b=none(len(q)), label=label)
        self._dev = None

    def _check_ids(self, qid, pos, neg, n_neg):
        """The first id, in the order the reference reads them (per line: query, positive, negatives), outside its cache."""
        nq, npas = len(self.query_cache), len(self.passage_cache)
        bad_q, bad_p, bad_n = (qid < 0) | (qid >= nq), (pos < 0) | (pos >= npas), (neg < 0) | (neg >= npas)
        if not (bad_q.any() or bad_p.any() or bad_n.any()):
            return
        line_of_neg = np.repeat(np.arange(len(n_neg)), n_neg)
        first = len(qid)
        for bad in (bad_q, bad_p):
            if bad.any():
                first = min(first, int(np.flatnonzero(bad)[0]))
        if bad_n.any():
            first = min(first, int(line_of_neg[np.flatnonzero(bad_n)[0]]))
        if bad_q[first]:
            key, size = qid[first], nq
        elif bad_p[first]:
            key, size = pos[first], npas
        else:
            key, size = neg[bad_n & (line_of_neg == first)][0], npas
        raise IndexError("Index {} is out of bound for cached embeddings of size {}".format(int(key), size))

    def draw_pass(self):
        """The plan of one pass.  MS MARCO forms: the fixed plan, nothing drawn.  DPR forms: one ``random.shuffle`` per kept line
        on the global ``random``, in line order, as the reference draws; the first negative after the shuffle is the item's."""
        if not self.dpr:
            return self.plan
        chosen = np.empty(len(self._qid), np.int64)
        for i, k in enumerate(self._n_neg.tolist()):
            order = list(range(k))
            random.shuffle(order)
            chosen[i] = order[0]
        neg = self._neg[self._neg_start + chosen]
        if self.triplet:
            n = len(neg)
            self.plan = dict(q=self._qid.copy(), a=self._pos.copy(), b=neg, label=np.full(n, -1, np.int64))
        else:
            q = np.repeat(self._qid, 2)
            a = np.empty(len(q), np.int64)
            a[0::2], a[1::2] = self._pos, neg
            self.plan = dict(q=q, a=a, b=np.full(len(q), -1, np.int64), label=np.full(len(q), -1, np.int64))
        self._dev = None
        return self.plan

    def __len__(self):
        return (self.n_items + self.batch_size - 1) // self.batch_size

    def _upload(self):
        import torch
        for c in (self.query_cache, self.passage_cache):
            if not isinstance(c, DeviceTokenCache):
                raise TypeError("iterating TrainingBatches needs DeviceTokenCache caches, got %s" % type(c).__name__)
        dev = self.passage_cache.device
        if self.query_cache.device != dev:
            raise ValueError("the two caches are on different devices")
        names = ["q", "a"] + (["b"] if self.triplet else []) + (["label"] if self.form == "msmarco_pair" else [])
        self._dev = {k: torch.from_numpy(np.ascontiguousarray(self.plan[k])).to(dev) for k in names}

    def __iter__(self):
        import torch
        self.draw_pass()
        if self._dev is None:
            self._upload()
        plan, n, B = self._dev, self.n_items, self.batch_size
        L = _lib.lib()
        dev = self.passage_cache.device
        mask_rule = _lib.GATHER_MASK_NONZERO if self.dpr else _lib.GATHER_MASK_LENGTH
        towers = [(self.query_cache, plan["q"], _lib.GATHER_TYPES_ZERO)]
        ptype = _lib.GATHER_TYPES_ZERO if self.dpr else _lib.GATHER_TYPES_LENGTH
        towers.append((self.passage_cache, plan["a"], ptype))
        if self.triplet:
            towers.append((self.passage_cache, plan["b"], ptype))
        segs = (_lib.AnceGatherSegment * len(towers))()
        for s, (cache, index, type_rule) in zip(segs, towers):
            s.d_records, s.n_records = cache.records.data_ptr(), len(cache)
            s.d_index, s.n_index = index.data_ptr(), n
            s.L, s.mask_rule, s.type_rule = cache.embedding_size, mask_rule, type_rule
        ids_dtype, mask_dtype = (torch.long, torch.long) if self.wide else (torch.int32, torch.bool)
        width = _lib.GATHER_WIDE if self.wide else _lib.GATHER_REFERENCE
        for first in range(0, n, B):
            b = min(B, n - first)
            out = []
            with torch.cuda.device(dev):  # per batch, not around the yield: the caller's current device is left alone
                for s, (cache, _, _) in zip(segs, towers):
                    shape = (b, cache.embedding_size)
                    trio = (torch.empty(shape, dtype=ids_dtype, device=dev), torch.empty(shape, dtype=mask_dtype, device=dev),
                            torch.empty(shape, dtype=torch.uint8, device=dev))
                    s.d_ids, s.d_mask, s.d_types = trio[0].data_ptr(), trio[1].data_ptr(), trio[2].data_ptr()
                    out.extend(trio)
                _lib.check(L.ance_gather_batch(segs, len(towers), first, b, width, _lib.current_stream_ptr()), "ance_gather_batch")
            if "label" in plan:
                out.append(plan["label"][first:first + b])
            yield tuple(out)
