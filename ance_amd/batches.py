"""The trainers' batches, assembled on the GPU from ``ann_training_data_N`` and the two token caches.

The reference builds them in one Python process, serial with the step (``DataLoader(..., batch_size=B)`` without workers over a
``StreamingDataset``: drivers/run_ann.py:199-208, drivers/run_ann_dpr.py:150-157): per item three ``seek`` + ``read`` calls on the
cache files (utils/util.py:292-298) and twelve ``torch.tensor(list_of_arrays)`` constructions (data/msmarco_data.py:275-362,
data/DPR_data.py:276-344), per batch default collation, nine host-to-device copies and six ``.long()`` casts
(drivers/run_ann.py:237-254).

Here the cache files are resident in HBM as their own bytes (``DeviceTokenCache``), the item list of the whole file (the *plan*:
which query, first passage and second passage every item reads) is parsed once and uploaded once, and a batch is ONE launch of
``ance_gather_batch`` (csrc/batch_gather.hip) on the current stream: no host-to-device copy, no synchronisation, no Python per item.

Packed batches: the lengths of all records are in the caches (``DeviceTokenCache.lengths``), so the plan also
carries the running sum of the sequence lengths (``TrainingBatches.cum``) and the exact token total of every batch
(``token_totals``).  ``TrainingBatches.packed(model)`` gathers a batch straight into one ``PackedTokens`` per tower with ONE launch of
``ance_gather_batch_packed`` (csrc/batch_gather_packed.hip), at capacities taken from the plan; ``PackedBatches.cursor()`` keeps the
position on the device, so the gather can be captured with the step.
"""
import json
import random

import numpy as np

from . import _lib

FORMS = ("msmarco_triplet", "msmarco_pair", "dpr_triplet", "dpr_pair")
UPLOAD_CHUNK_BYTES = 64 << 20
MAX_CHUNK_LEN, MAX_SEQS = 512, 65535   # packing.MAX_SEQ_LEN, packing.MAX_SEQS (not imported here: the plan needs no torch)


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

    def lengths(self, chunk_len=None, rule=_lib.GATHER_MASK_LENGTH):
        """int32 device tensor [N, L / chunk_len]: the length of every chunk of every record (``ance_record_lengths``, one launch, made
        once and kept).  ``rule``: ``_lib.GATHER_MASK_LENGTH`` -- the header, clamped to L and spread over the chunks -- or
        ``_lib.GATHER_MASK_NONZERO`` -- the non-zero ids of the chunk (the DPR loaders' mask).  ``chunk_len`` defaults to L; it must
        divide L and be at most 512."""
        import torch
        chunk_len = _check_chunk_len(self.embedding_size if chunk_len is None else chunk_len, self.embedding_size, self.base_path)
        _check_rule(rule)
        made = self.__dict__.setdefault("_lengths", {})
        if (chunk_len, rule) not in made:
            out = torch.empty((self.total_number, self.embedding_size // chunk_len), dtype=torch.int32, device=self.device)
            if self.total_number:
                with torch.cuda.device(self.device):
                    _lib.check(_lib.lib().ance_record_lengths(self.records.data_ptr(), self.total_number, self.embedding_size, chunk_len,
                                                              rule, out.data_ptr(), _lib.current_stream_ptr()), "ance_record_lengths")
            made[(chunk_len, rule)] = out
        return made[(chunk_len, rule)]


def _check_chunk_len(chunk_len, L, what):
    if isinstance(chunk_len, bool) or not isinstance(chunk_len, (int, np.integer)) or chunk_len < 1:
        raise ValueError("chunk_len %r: an int >= 1" % (chunk_len,))
    if L % chunk_len:
        raise ValueError("chunk_len %d does not divide the %d tokens of a record of %s" % (chunk_len, L, what))
    if chunk_len > MAX_CHUNK_LEN:
        raise ValueError("chunk_len %d of %s is above %d, the longest sequence a tower takes" % (chunk_len, what, MAX_CHUNK_LEN))
    return int(chunk_len)


def _check_rule(rule):
    if rule not in (_lib.GATHER_MASK_LENGTH, _lib.GATHER_MASK_NONZERO):
        raise ValueError("rule %r: _lib.GATHER_MASK_LENGTH or _lib.GATHER_MASK_NONZERO" % (rule,))


def record_lengths(cache, chunk_len, rule):
    """int32 torch tensor [N, L / chunk_len] of a cache's chunk lengths: ``DeviceTokenCache.lengths`` on the cache's device, or, for a
    host ``TokenCache``, the same numbers from NumPy on the CPU (the plan and its totals need no GPU)."""
    import torch
    if isinstance(cache, DeviceTokenCache):
        return cache.lengths(chunk_len, rule)
    L = cache.embedding_size
    chunk_len = _check_chunk_len(chunk_len, L, cache.base_path)
    _check_rule(rule)
    if rule == _lib.GATHER_MASK_LENGTH:
        whole = cache.lengths().astype(np.int64)
        out = np.clip(whole[:, None] - np.arange(L // chunk_len)[None, :] * chunk_len, 0, chunk_len)
    else:
        out = (cache.ids().reshape(len(cache), L // chunk_len, chunk_len) != 0).sum(2)
    return torch.from_numpy(np.ascontiguousarray(out, np.int32))


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

    Packed batches: ``cum(name)`` is the running sum of a tower's sequence lengths over the pass, ``token_totals()`` the exact
    token count of every batch, ``max_token_totals()`` a bound for every pass; all three work with host caches and no GPU.
    ``packed(model)`` returns the ``PackedBatches`` that gathers straight into packed rows.
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
        self._cums, self._totals, self._max_totals = {}, None, None   # the packed plan: cum per (tower, chunk_len), the totals

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
        self._cums, self._totals = {}, None   # of the pass before; the "max" totals hold for every pass
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

    # ---------------------------------------------------------------------------------------------------------- the packed plan
    def tower_names(self):
        """The plan keys of the form's towers, in the tuple's order: q, a and, for a triplet form, b."""
        return ("q", "a", "b") if self.triplet else ("q", "a")

    def _tower_cache(self, name):
        return self.query_cache if name == "q" else self.passage_cache

    def _on_device(self):
        return isinstance(self.query_cache, DeviceTokenCache) or isinstance(self.passage_cache, DeviceTokenCache)

    def _length_rule(self):
        return _lib.GATHER_MASK_NONZERO if self.dpr else _lib.GATHER_MASK_LENGTH

    def _chunk_len(self, name, chunk_len):
        """The sequence length of a tower: the query's is its record; a body's is chunk_len, by default the record, or 512 where
        the record is longer (a MaxP document)."""
        L = self._tower_cache(name).embedding_size
        if name == "q" or chunk_len is None:
            chunk_len = L if name == "q" or L <= MAX_CHUNK_LEN else MAX_CHUNK_LEN
        return _check_chunk_len(chunk_len, L, self._tower_cache(name).base_path)

    def _index(self, name):
        """The int64 record index of a tower's items where the plan lives: on the caches' device, or on the CPU for host caches."""
        import torch
        if self.plan is None:
            raise ValueError("the %s form has no plan before a pass is drawn: call draw_pass() or iterate first" % self.form)
        if self._on_device():
            if self._dev is None:
                self._upload()
            return self._dev[name]
        return torch.from_numpy(np.ascontiguousarray(self.plan[name]))

    def cum(self, name, chunk_len=None):
        """int64 [n_items * C + 1] where the plan lives: the exclusive running sum of the lengths of tower ``name``'s sequences of
        this pass in item-then-chunk order (C = L / chunk_len chunks per item).  Built with torch ops once per pass and kept; the
        DPR forms rebuild it with every drawn pass.  This is the scan ``ance_pack_tokens`` does per call, done at plan time."""
        import torch
        chunk_len = self._chunk_len(name, chunk_len)
        key = (name, chunk_len)
        if key not in self._cums:
            index = self._index(name)
            per = record_lengths(self._tower_cache(name), chunk_len, self._length_rule())[index].reshape(-1)
            cum = torch.zeros(per.numel() + 1, dtype=torch.int64, device=per.device)
            torch.cumsum(per, 0, dtype=torch.int64, out=cum[1:])
            self._cums[key] = cum
        return self._cums[key]

    def _batch_bounds(self):
        n, B = self.n_items, self.batch_size
        return np.minimum(np.arange(0, n + B, B, dtype=np.int64)[:len(self) + 1], n)

    def token_totals(self, chunk_len=None):
        """int64 array [len(self), n_towers]: the exact token count of every batch of this pass, per tower in ``tower_names()``
        order -- what ``"exact"`` and ``"max"`` capacities are made of.  One read-back, made once per pass and kept; never inside a
        step.  The totals do not depend on chunk_len (a record's chunks sum to its length); it only names the ``cum`` to use."""
        import torch
        if self._totals is None:
            cols = []
            for name in self.tower_names():
                cum = self.cum(name, chunk_len)
                C = self._tower_cache(name).embedding_size // self._chunk_len(name, chunk_len)
                ends = cum[torch.from_numpy(self._batch_bounds() * C).to(cum.device)]
                cols.append(ends[1:] - ends[:-1])
            self._totals = torch.stack(cols, 1).cpu().numpy().astype(np.int64).reshape(len(self), len(cols))
        return self._totals

    def max_token_totals(self):
        """[n_towers] ints: per tower a token count no batch exceeds.  MS MARCO forms: the maximum over ``token_totals()``.  DPR
        forms: the maximum over the batches with every line's negative counted at the line's LONGEST one, so it holds for every draw
        of every pass (no pass needs to be drawn for it)."""
        import torch
        if self._max_totals is None:
            if not self.dpr:
                t = self.token_totals()
                self._max_totals = [int(t[:, k].max()) if len(t) else 0 for k in range(t.shape[1])]
            else:
                rule, bounds = self._length_rule(), self._batch_bounds()
                whole = {c: record_lengths(c, self._chunk_len(n, None), rule).sum(1, dtype=torch.int64)
                         for n, c in (("q", self.query_cache), ("a", self.passage_cache))}
                dev = whole[self.passage_cache].device
                at = lambda cache, ids: whole[cache][torch.from_numpy(np.ascontiguousarray(ids)).to(dev)]  # noqa: E731
                q, pos = at(self.query_cache, self._qid), at(self.passage_cache, self._pos)
                worst = torch.zeros(len(self._qid), dtype=torch.int64, device=dev)
                line_of_neg = torch.from_numpy(np.repeat(np.arange(len(self._n_neg)), self._n_neg)).to(dev)
                worst.scatter_reduce_(0, line_of_neg, at(self.passage_cache, self._neg), "amax", include_self=True)
                if self.triplet:
                    per_item = [q, pos, worst]
                else:
                    per_item = [q.repeat_interleave(2), torch.stack([pos, worst], 1).reshape(-1)]
                sums = []
                for per in per_item:
                    cum = torch.zeros(per.numel() + 1, dtype=torch.int64, device=dev)
                    torch.cumsum(per, 0, out=cum[1:])
                    ends = cum[torch.from_numpy(bounds).to(dev)]
                    sums.append((ends[1:] - ends[:-1]).max() if len(self) else torch.zeros((), dtype=torch.int64, device=dev))
                self._max_totals = [int(v) for v in torch.stack(sums).cpu()]
        return list(self._max_totals)

    def packed(self, model, query_rows="max", body_rows="max", chunk_len=None):
        """A ``PackedBatches`` over the same item stream: per batch one ``PackedTokens`` per tower, gathered straight from the caches
        by ONE launch (see ``PackedBatches``)."""
        return PackedBatches(self, model, query_rows, body_rows, chunk_len)

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


def _check_rows(rows, what):
    if rows in ("max", "exact"):
        return rows
    if isinstance(rows, bool) or not isinstance(rows, (int, np.integer)) or not 1 <= rows <= 0x7fffffff:
        raise ValueError("%s %r: \"max\", \"exact\" or an int capacity in 1 .. 2^31 - 1" % (what, rows))
    return int(rows)


class PackedBatches:
    """``TrainingBatches.packed(model, query_rows="max", body_rows="max", chunk_len=None)``: the same item stream as packed token
    rows.  Iterating yields, per batch, one ``PackedTokens`` per tower in the padded tuple's tower order -- (q, a, b) for a triplet
    form, (q, a) for a pair form, and the label slice last for ``msmarco_pair`` -- that the model's ``forward`` / ``query_emb`` /
    ``body_emb`` take in place of ``input_ids`` (``attention_mask=None``).  Each batch is ONE launch of ``ance_gather_batch_packed``
    on the current stream: no padded ids, no mask, no ``lens_from_mask``, no pack, no copy, no synchronisation.  No token types
    are produced (``type_ids`` is None): no model here passes them to a tower.

    The position rule, pad id and table sizes are the model's: its query tower's for the query segment, its body tower's for the
    others.  ``chunk_len``: the body's sequence length, by default ``model.base_len`` where the model has one (MaxP: a document is
    L / chunk_len sequences, ``PackedTokens.chunks`` says how many) and the record otherwise.

    Capacities (``query_rows`` for the query tower, ``body_rows`` for every body tower):
      an int    used as given; a sequence that does not fit is dropped (its embedding is NaN, ``dropped`` counts it)
      "exact"   the batch's own total from ``token_totals()``, at least 1: shapes vary per batch, nothing synchronises; for eager use
      "max"     ONE int for the whole object that no batch exceeds (``max_token_totals()``; the DPR forms count every line at its
                longest negative, so it holds for every draw of every pass and a captured graph survives ``iter()``)
    ``capacity`` is the pair (query, body) of ints, None where "exact".

    ``cursor()`` gives the capturable form: fixed output buffers and the position on the device."""

    def __init__(self, batches, model, query_rows="max", body_rows="max", chunk_len=None):
        tb = self.batches = batches
        names = tb.tower_names()
        if chunk_len is None:
            chunk_len = getattr(model, "base_len", None)
        self.chunk_len = {n: tb._chunk_len(n, chunk_len) for n in names}
        self.chunks = {n: tb._tower_cache(n).embedding_size // self.chunk_len[n] for n in names}
        if tb.batch_size * max(self.chunks.values()) > MAX_SEQS:
            raise ValueError("batch_size %d x %d chunks is above the %d sequences a packed batch holds"
                             % (tb.batch_size, max(self.chunks.values()), MAX_SEQS))
        rows = (_check_rows(query_rows, "query_rows"), _check_rows(body_rows, "body_rows"))
        for c in (tb.query_cache, tb.passage_cache):
            if not isinstance(c, DeviceTokenCache):
                raise TypeError("packed batches need DeviceTokenCache caches, got %s" % type(c).__name__)
        self.device = tb.passage_cache.device
        if tb.query_cache.device != self.device:
            raise ValueError("the two caches are on different devices")
        towers = model.towers()
        for t in towers:
            dev = t.embeddings.word_embeddings.weight.device
            if dev != self.device:
                raise ValueError("the model is on %s, the token caches on %s" % (dev, self.device))
        self.rules = {n: towers[0 if n == "q" else 1].embeddings.pack_rule for n in names}
        if "max" in rows:
            most = tb.max_token_totals()
            most = (max(1, most[0]), max(1, max(most[1:])))
            rows = tuple(m if r == "max" else r for r, m in zip(rows, most))
        self._rows = rows
        self.capacity = tuple(None if r == "exact" else r for r in rows)
        model._dropped_counter(self.device)   # here, not inside a step: a captured step only adds

    def __len__(self):
        return len(self.batches)

    def _segments(self, index, cum):
        tb = self.batches
        names = tb.tower_names()
        segs = (_lib.AncePackedGatherSegment * len(names))()
        for s, n in zip(segs, names):
            cache, rule = tb._tower_cache(n), self.rules[n]
            s.d_records, s.n_records = cache.records.data_ptr(), len(cache)
            s.d_index, s.n_index, s.d_cum = index[n].data_ptr(), tb.n_items, cum[n].data_ptr()
            s.L, s.chunk_len = cache.embedding_size, self.chunk_len[n]
            s.position_mode, s.padding_idx = _lib.EMBED_POSITION_MODES[rule.position_mode], rule.padding_idx
            s.vocab, s.max_pos = rule.vocab, rule.max_pos
        return segs

    def _outputs(self, segs, b, rows):
        """Fresh outputs of a batch of b items with the capacity of every tower, wired into the segment table."""
        import torch
        from .packing import PackedTokens
        out = []
        for s, n, R in zip(segs, self.batches.tower_names(), rows):
            n_seq = b * self.chunks[n]
            i32 = lambda k: torch.empty(k, dtype=torch.int32, device=self.device)  # noqa: E731
            p = PackedTokens(i32(R), None, i32(R), i32(n_seq + 1), i32(n_seq), R, self.chunk_len[n],
                             torch.empty((), dtype=torch.int64, device=self.device), self.rules[n], self.chunks[n])
            s.packed_ids, s.packed_positions, s.rows = p.ids.data_ptr(), p.positions.data_ptr(), R
            s.d_seq_off, s.d_seq_kept, s.d_dropped = p.seq_off.data_ptr(), p.seq_kept.data_ptr(), p.dropped.data_ptr()
            out.append(p)
        return out

    def _plan_tensors(self):
        tb = self.batches
        names = tb.tower_names()
        return {n: tb._index(n) for n in names}, {n: tb.cum(n, self.chunk_len[n]) for n in names}

    def __iter__(self):
        import torch
        tb = self.batches
        tb.draw_pass()
        if not len(tb):
            return
        index, cum = self._plan_tensors()
        segs = self._segments(index, cum)
        n, B, L = tb.n_items, tb.batch_size, _lib.lib()
        totals = tb.token_totals() if "exact" in self._rows else None
        label = tb._dev.get("label")
        for k, first in enumerate(range(0, n, B)):
            b = min(B, n - first)
            rows = [self._rows[0 if j == 0 else 1] for j in range(len(segs))]
            rows = [max(1, int(totals[k, j])) if r == "exact" else r for j, r in enumerate(rows)]
            with torch.cuda.device(self.device):
                out = self._outputs(segs, b, rows)
                _lib.check(L.ance_gather_batch_packed(segs, len(segs), first, b, None, _lib.current_stream_ptr()),
                           "ance_gather_batch_packed")
            if label is not None:
                out.append(label[first:first + b])
            yield tuple(out)

    def cursor(self):
        """A ``PackedCursor`` over this object's item stream (int capacities only: "exact" has no fixed shape)."""
        return PackedCursor(self)


class PackedCursor:
    """The capturable form of ``PackedBatches``: fixed output buffers and a position that lives on the device.

      .batch      one ``PackedTokens`` per tower, allocated once; every ``next()`` overwrites them
      .labels     ``msmarco_pair`` only: int64 [B], the labels of the batch (None otherwise)
      .position   int64 device scalar: the first item of the next batch
      .n_full     n_items // B, the number of whole batches
      .next()     ONE launch of the gather reading ``position`` on the device, then ``position.add_(B)`` on the same stream; both
                  can be captured, so a graph that holds ``next()``, forward, backward and the optimizer walks the pass by replaying.
                  Returns ``.batch``
      .reset()    copies the CURRENT pass's plan of the TrainingBatches into the cursor's own (fixed) plan buffers and writes the
                  position back to 0: after ``draw_pass()`` of a DPR form a captured graph goes on with the new pass

    A batch always has B items.  Items at or beyond the end of the plan are EMPTY sequences (``seq_kept`` 0, no rows), whatever the
    position holds; nothing is read outside the plan.  The short last batch of a pass (n_items % B items) is therefore NOT served
    here as the iteration serves it: iterate it eagerly (``PackedBatches.__iter__`` yields it last) or drop it."""

    def __init__(self, packed):
        import torch
        self.packed, tb = packed, packed.batches
        if None in packed.capacity:
            raise ValueError("a cursor needs int or \"max\" capacities: \"exact\" has no fixed shape")
        if tb.plan is None:
            tb.draw_pass()
        self.n_full = tb.n_items // tb.batch_size
        index, cum = packed._plan_tensors()
        self._index, self._cum = {n: t.clone() for n, t in index.items()}, {n: t.clone() for n, t in cum.items()}
        self._segs = packed._segments(self._index, self._cum)
        rows = [packed.capacity[0 if j == 0 else 1] for j in range(len(self._segs))]
        with torch.cuda.device(packed.device):
            self.batch = tuple(packed._outputs(self._segs, tb.batch_size, rows))
            self.position = torch.zeros((), dtype=torch.int64, device=packed.device)
            self._label = tb._dev["label"].clone() if "label" in tb._dev else None
            self.labels = None
            if self._label is not None:
                self.labels = torch.zeros(tb.batch_size, dtype=torch.int64, device=packed.device)
                self._ar = torch.arange(tb.batch_size, dtype=torch.int64, device=packed.device)

    def reset(self):
        tb = self.packed.batches
        index, cum = self.packed._plan_tensors()
        for mine, theirs in ((self._index, index), (self._cum, cum)):
            for n, t in mine.items():
                t.copy_(theirs[n])
        if self._label is not None:
            self._label.copy_(tb._dev["label"])
        self.position.zero_()
        return self

    def next(self):
        import torch
        tb = self.packed.batches
        with torch.cuda.device(self.packed.device):
            _lib.check(_lib.lib().ance_gather_batch_packed(self._segs, len(self._segs), 0, tb.batch_size, self.position.data_ptr(),
                                                           _lib.current_stream_ptr()), "ance_gather_batch_packed")
            if self._label is not None and tb.n_items:
                torch.index_select(self._label, 0, (self.position + self._ar).clamp_(0, tb.n_items - 1), out=self.labels)
            self.position.add_(tb.batch_size)
        return self.batch
