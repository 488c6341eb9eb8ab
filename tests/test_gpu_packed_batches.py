"""Packed training batches on the GPU (ance_amd.batches.PackedBatches / PackedCursor -> csrc/batch_gather_packed.hip; INTEGRATION.md
3o).  Every comparison is bit for bit, and the oracle is the path that exists already: ``pack_tokens`` applied to the padded batch
``TrainingBatches`` gathers (``lens_from_mask`` of its mask), on the same device.

  record lengths   both caches of every batches_util case, both rules, chunk_len = L where a tower takes L (<= 512), and the maxp
                   documents at 512 (3 x 2048 -> 4 chunks), against NumPy; the 2048-token chunk is refused
  gather           batches_util.combos() x batch sizes 1 / 5 / 64 x both position rules, capacities per tower "exact", total + 5,
                   total - 1, 1 and B * L: ids, positions, seq_off, seq_kept and the dropped count, the slack rows included, with a
                   guard band of 64 int32 behind every output; `small` also with vocab 1000 and max_pos 10, where the clamps act
  cursor           n_full batches by next() equal the iteration; a cursor at n_items - 1, n_items and n_items + 10 B yields empty
                   sequences for the missing items -- a bounds contract checked on the results
  determinism      two calls give equal bytes; `dropped` is this batch's count per segment, not accumulated, not mixed
  model            loss and every gradient of model(q, None, a, None, b, None) on a packed batch equal set_packed_rows(Rq, Rb) on the
                   padded batch with the same R: dropout 0 and 0.1, fp32 and precision="half" under bf16 autocast; one MaxP case
  capture          one graph holds cursor.next(), forward, backward and Lamb.step(); replayed on three consecutive batches it equals
                   three eager steps fed by iterating the same PackedBatches
"""
import random

import numpy as np
import pytest
import torch

import batches_util as U
import lamb_util as LU
import model_util as M
import packed_batches_util as PB
import train_step_util as S
from ance_amd import _lib
from ance_amd.cache import TokenCache

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
POISON = {torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A}
RULES = (("roberta", 1, 30522, 514), ("absolute", 0, 30522, 514))
CLAMPED_RULES = (("roberta", 1, 1000, 10), ("absolute", 0, 1000, 10))   # ids reach 30000, columns reach 20: both clamps act


@pytest.fixture(autouse=True)
def _host_mode_afterwards():
    from ance_amd import attention as T
    yield
    T.dropout_state.to_host(0)
    T.manual_seed(S.SEED)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    from ance_amd.batches import DeviceTokenCache
    d = str(tmp_path_factory.mktemp("packed_batches"))
    out = {}
    for case in U.CASES:
        qp, pp, lines = U.build_case(case, d)
        out[case] = (DeviceTokenCache(qp, DEV), DeviceTokenCache(pp, DEV), lines, TokenCache(qp), TokenCache(pp))
    return out


class _Embeddings(object):
    def __init__(self, rule):
        from ance_amd.packing import PackRule
        self.pack_rule = PackRule.of(*rule)
        self.word_embeddings = torch.nn.Embedding(1, 1).to(DEV)


class _Rules(object):
    """What PackedBatches reads of a model: the towers' rules and device, and the dropped counter."""

    def __init__(self, rule):
        self.tower = type("Tower", (), {})()
        self.tower.embeddings = _Embeddings(rule)
        self.packed_dropped = None

    def towers(self):
        return self.tower, self.tower

    def _dropped_counter(self, dev):
        self.packed_dropped = torch.zeros((), dtype=torch.int64, device=dev)
        return self.packed_dropped


def make(cases, case, form, world=1, rank=0, batch_size=4, dtype=None):
    from ance_amd.batches import TrainingBatches
    qc, pc, lines = cases[case][:3]
    c = U.CASES[case]
    return TrainingBatches(lines, qc, pc, batch_size, form, c["L_q"], c["L_p"], rank=rank, world_size=world, dtype=dtype)


def _chunk(case):
    return 512 if case == "maxp" else None


# ---------------------------------------------------------------------------------------------------------------- record lengths
@pytest.mark.parametrize("case", list(U.CASES))
def test_record_lengths_against_numpy(cases, case):
    qc, pc, _, hq, hp = cases[case]
    for dev_cache, host in ((qc, hq), (pc, hp)):
        L = host.embedding_size
        whole = host.lengths().astype(np.int64)
        if len(host) >= 4:
            assert {0, 1, L - 1, L} <= set(whole.tolist())
        for ch in ([L] if L <= 512 else []) + ([512] if L > 512 else []):
            C = L // ch
            want = {_lib.GATHER_MASK_LENGTH: np.clip(whole[:, None] - np.arange(C)[None, :] * ch, 0, ch),
                    _lib.GATHER_MASK_NONZERO: (host.ids().reshape(len(host), C, ch) != 0).sum(2)}
            for rule, w in want.items():
                got = dev_cache.lengths(None if ch == L else ch, rule)
                assert got.dtype == torch.int32 and tuple(got.shape) == (len(host), C) and got.device == dev_cache.device
                assert np.array_equal(got.cpu().numpy(), w.astype(np.int32)), (case, ch, rule)
                assert dev_cache.lengths(ch, rule) is got                      # made once
        if L > 512:
            with pytest.raises(ValueError, match="above 512"):
                dev_cache.lengths()
            L_ = _lib.lib()
            out = torch.zeros(len(host), dtype=torch.int32, device=DEV)
            assert L_.ance_record_lengths(dev_cache.records.data_ptr(), len(host), L, L, 0, out.data_ptr(), None) == -1
    if case == "dpr":   # passage 4: ten tokens, the fourth of them 0
        assert int(pc.lengths(rule=_lib.GATHER_MASK_LENGTH)[4]) == 10 and int(pc.lengths(rule=_lib.GATHER_MASK_NONZERO)[4]) == 9


# ---------------------------------------------------------------------------------------------------------------- the gather
def _guarded(n, dtype=torch.int32):
    """n elements with a guard band of 64 int32 (32 int64) behind them, all poisoned."""
    return torch.full((n + (GUARD if dtype == torch.int32 else GUARD // 2),), POISON[dtype], dtype=dtype, device=DEV)


def _launch(pb, segs, b, rows, first=0, d_first=None):
    """One ance_gather_batch_packed call into poisoned buffers: ([ids, positions, seq_off, seq_kept, dropped] per tower, one flag per
    buffer saying that its guard band still holds the poison)."""
    outs, guards = [], []
    for s, n, R in zip(segs, pb.batches.tower_names(), rows):
        n_seq = b * pb.chunks[n]
        sizes = (R, R, n_seq + 1, n_seq, 1)
        bufs = [_guarded(R), _guarded(R), _guarded(n_seq + 1), _guarded(n_seq), _guarded(1, torch.int64)]
        s.packed_ids, s.packed_positions, s.d_seq_off, s.d_seq_kept, s.d_dropped = (t.data_ptr() for t in bufs)
        s.rows = R
        outs.append([t[:k] for t, k in zip(bufs, sizes)])
        guards += [(t, k) for t, k in zip(bufs, sizes)]
    rc = _lib.lib().ance_gather_batch_packed(segs, len(segs), first, b, d_first, _lib.current_stream_ptr())
    assert rc == 0, _lib.lib().ance_last_error()
    return outs, [(t[k:] == POISON[t.dtype]).all() for t, k in guards]


def _oracle(padded, j, C, ch, R, rule):
    """pack_tokens of tower j's share of a padded batch (TrainingBatches' tuple) at capacity R."""
    from ance_amd.attention import lens_from_mask
    from ance_amd.packing import pack_tokens
    ids, mask = padded[3 * j], padded[3 * j + 1]
    return pack_tokens(ids.reshape(-1, ch), lens_from_mask(mask.reshape(-1, ch)), R, None, rule[0], rule[1], rule[2], rule[3])


def _same(got, want):
    """Flags: the five outputs of a tower against a PackedTokens."""
    return [torch.equal(got[0], want.ids), torch.equal(got[1], want.positions), torch.equal(got[2], want.seq_off),
            torch.equal(got[3], want.seq_kept), int(got[4][0]) == int(want.dropped)]


def _gather_params():
    out = []
    for case, form, world, rank in U.combos():
        for rule in RULES + (CLAMPED_RULES if case == "small" else ()):
            out.append(pytest.param(case, form, world, rank, rule, id="%s-%s-%d" % (U.key(case, form, world, rank), rule[0], rule[3])))
    return out


@pytest.mark.parametrize("case,form,world,rank,rule", _gather_params())
def test_gather_equals_pack_tokens_of_the_padded_gather(cases, case, form, world, rank, rule):
    """Every batch of the pass at five capacities per tower.  total - 1 drops the last non-empty sequence and the empty ones behind
    it; 1 drops nearly everything; batch size 64 is one short batch (the plan holds fewer items)."""
    model = _Rules(rule)
    for B in U.BATCH_SIZES:
        random.seed(U.DPR_SEED)
        tb = make(cases, case, form, world, rank, B)
        pb = tb.packed(model, chunk_len=_chunk(case))
        padded = list(tb)                      # draws the pass; PackedBatches' own iteration is not used here, so no second draw
        totals = tb.token_totals(_chunk(case))
        names = tb.tower_names()
        index, cum = pb._plan_tensors()
        segs = pb._segments(index, cum)
        assert len(padded) == len(tb) == len(totals) and (B != 64 or (len(tb) == 1 and tb.n_items < 64))
        for k, batch in enumerate(padded):
            first, b = k * B, batch[0].shape[0]
            for what in ("exact", "slack", "short", "one", "full"):
                rows = []
                for j, n in enumerate(names):
                    t, full = int(totals[k, j]), b * tb._tower_cache(n).embedding_size
                    rows.append(dict(exact=max(1, t), slack=t + 5, short=max(1, t - 1), one=1, full=full)[what])
                outs, guards = _launch(pb, segs, b, rows, first)
                for j, n in enumerate(names):
                    want = _oracle(batch, j, pb.chunks[n], pb.chunk_len[n], rows[j], rule)
                    same = _same(outs[j], want)
                    assert all(same), (B, k, what, n, rows[j], same)
                    if what == "short" and totals[k, j] > 1:
                        assert int(want.dropped) >= 1
                assert bool(torch.stack(guards).all()), (B, k, what, "a guard band was written")


@pytest.mark.parametrize("case,form", [("small", "msmarco_pair"), ("maxp", "msmarco_triplet"), ("dpr", "dpr_triplet"), ("dpr", "dpr_pair")])
def test_iteration_yields_the_same_batches(cases, case, form):
    """The public iteration: "exact", "max" and int capacities; the PackedTokens' host fields; the labels of msmarco_pair."""
    rule = RULES[0]
    model = _Rules(rule)
    for B in (5, 64):
        tb = make(cases, case, form, batch_size=B)
        for q_rows, b_rows in (("exact", "exact"), ("max", "max"), (7, "max")):
            pb = tb.packed(model, q_rows, b_rows, chunk_len=_chunk(case))
            random.seed(U.DPR_SEED)
            padded = list(tb)
            random.seed(U.DPR_SEED)
            got = list(pb)
            totals = tb.token_totals(_chunk(case))
            if q_rows == "max":
                want_cap = (max(1, int(totals[:, 0].max())), max(1, int(totals[:, 1:].max())))
                assert pb.capacity[0] >= want_cap[0] and pb.capacity[1] >= want_cap[1]
                assert form.startswith("dpr") or pb.capacity == want_cap
            assert len(got) == len(padded) == len(pb)
            for k, (batch, pk) in enumerate(zip(padded, got)):
                names = tb.tower_names()
                assert len(pk) == len(names) + (form == "msmarco_pair")
                for j, n in enumerate(names):
                    p = pk[j]
                    R = max(1, int(totals[k, j])) if (q_rows if j == 0 else b_rows) == "exact" else pb.capacity[0 if j == 0 else 1]
                    assert p.rows == R == p.ids.numel() and p.type_ids is None and p.chunks == pb.chunks[n]
                    assert p.max_seq_len == pb.chunk_len[n] and p.rule == model.tower.embeddings.pack_rule
                    want = _oracle(batch, j, pb.chunks[n], pb.chunk_len[n], R, rule)
                    assert all(_same([p.ids, p.positions, p.seq_off, p.seq_kept, p.dropped.reshape(1)], want)), (B, k, n)
                if form == "msmarco_pair":
                    assert torch.equal(pk[-1], batch[-1])


# ---------------------------------------------------------------------------------------------------------------- the cursor
@pytest.mark.parametrize("case,form", [("small", "msmarco_triplet"), ("maxp", "msmarco_pair"), ("dpr", "dpr_pair")])
def test_cursor_walks_the_pass_and_stays_inside_the_plan(cases, case, form):
    rule = RULES[0] if case != "dpr" else RULES[1]
    model = _Rules(rule)
    B = 5
    tb = make(cases, case, form, batch_size=B)
    pb = tb.packed(model, chunk_len=_chunk(case))
    random.seed(U.DPR_SEED)
    want = [[(p.ids.clone(), p.positions.clone(), p.seq_off.clone(), p.seq_kept.clone(), p.dropped.clone()) for p in pk[:len(tb.tower_names())]]
            + [pk[-1].clone() if form == "msmarco_pair" else None] for pk in pb]
    cur = pb.cursor()           # the plan of the pass just drawn
    assert cur.n_full == tb.n_items // B and cur.n_full >= 2 and int(cur.position) == 0
    buffers = [p.ids.data_ptr() for p in cur.batch]
    for k in range(cur.n_full):
        got = cur.next()
        assert got is cur.batch and [p.ids.data_ptr() for p in got] == buffers
        for j, p in enumerate(got):
            for a, b in zip((p.ids, p.positions, p.seq_off, p.seq_kept, p.dropped), want[k][j]):
                assert torch.equal(a, b), (k, j)
        if form == "msmarco_pair":
            assert torch.equal(cur.labels, want[k][-1])
        assert int(cur.position) == (k + 1) * B
    # beyond the plan: the missing items are empty sequences, whatever the position holds
    host = cases[case][3:]
    towers = PB.tower_batches(form, tb.plan, host[0], host[1], _chunk(case))
    n = tb.n_items
    for position in (n - 1, n, n + 10 * B):
        cur.position.fill_(position)
        got = cur.next()
        assert int(cur.position) == position + B
        for j, (name, tower) in enumerate(towers.items()):
            here = max(0, min(B, n - position))
            R = pb.capacity[0 if j == 0 else 1]
            w = PB.packed_batch(tower, min(position, n), here, R, rule[0], rule[1], rule[2], rule[3], missing=B - here)
            p, C = got[j], tower[2]
            assert np.array_equal(p.seq_kept.cpu().numpy(), w["seq_kept"]) and (w["seq_kept"][here * C:] == 0).all()
            assert np.array_equal(p.seq_off.cpu().numpy(), w["seq_off"]) and int(p.seq_off[-1]) == w["T"]
            assert np.array_equal(p.ids.cpu().numpy(), w["ids"]) and np.array_equal(p.positions.cpu().numpy(), w["positions"])
            assert int(p.dropped) == 0
            if here == 0:
                assert w["T"] == 0 and not p.seq_kept.any()
    assert int(cur.reset().position) == 0
    got = cur.next()
    assert all(torch.equal(p.ids, w[0]) for p, w in zip(got, want[0]))


# ---------------------------------------------------------------------------------------------------------------- determinism
def test_two_calls_give_equal_bytes_and_dropped_is_this_batch_s_count(cases):
    """Only the query tower drops (capacity 3 against full body capacities): its count is the batch's own in both calls -- stored,
    not accumulated -- and the body segments' stay 0."""
    rule = RULES[0]
    B = 5
    tb = make(cases, "small", "msmarco_triplet", batch_size=B)
    pb = tb.packed(_Rules(rule), query_rows=3, body_rows=B * 20)
    cur = pb.cursor()
    padded = list(tb)
    runs = []
    for _ in range(2):
        cur.position.fill_(B)
        got = cur.next()
        runs.append([[t.clone() for t in (p.ids, p.positions, p.seq_off, p.seq_kept, p.dropped)] for p in got])
    for a, b in zip(*runs):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    want = [_oracle(padded[1], j, 1, (8, 20, 20)[j], (3, B * 20, B * 20)[j], rule) for j in range(3)]
    dropped = [int(r[4]) for r in runs[1]]
    assert dropped == [int(w.dropped) for w in want] and dropped[0] >= 1 and dropped[1:] == [0, 0]
    for r, w in zip(runs[1], want):
        assert all(_same([r[0], r[1], r[2], r[3], r[4].reshape(1)], w))


# ---------------------------------------------------------------------------------------------------------------- the model
def _write_model_caches(directory, name, pad, n_p, L_p, n_q, L_q):
    """batches_util's caches with the ids taken modulo the small models' vocabulary (pad after the length)."""
    paths = []
    for what, n, L, seed in (("queries", n_q, L_q, 311), ("passages", n_p, L_p, 312)):
        lens, ids = U.cache_arrays(n, L, pad, seed)
        ids = np.where(np.arange(L)[None, :] < lens[:, None], 2 + ids % (S.VOCAB - 2), pad).astype(np.int32)
        base = "%s/%s_%s" % (directory, name, what)
        U.write_cache(base, lens, ids)
        paths.append(base)
    return paths


def _config(cfg, p):
    from ance_amd.model import TowerConfig
    return TowerConfig(S.VOCAB, cfg["H"], cfg["N"], cfg["inter"], S.MAX_POS, cfg["n_types"], cfg["eps"], cfg["pad"], p, p, cfg["heads"])


def _load(model, sd):
    return model.to(DEV).load_reference_state_dict({k: torch.from_numpy(np.ascontiguousarray(v, np.float32)) for k, v in sd.items()})


def _model(which, p, precision="fp32"):
    from ance_amd import model
    if which == "base_biencoder":
        sd = {}
        for pre, seed in (("question_model.", 73), ("ctx_model.", 74)):
            sd.update({k: v for k, v in M.model_state(S.BASE, seed, prefix=pre).items() if k.startswith(pre)})
        return _load(model.BiEncoder(_config(S.BASE, p), precision=precision), sd).train()
    cls = model.RobertaDot_NLL_LN if which == "large_roberta_dot" else model.RobertaDot_CLF_ANN_NLL_MultiChunk
    return _load(cls(_config(S.LARGE, p), precision=precision), M.model_state(S.LARGE)).train()


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).contiguous().view(torch.uint8),
                                                                           b.reshape(-1).contiguous().view(torch.uint8))


@pytest.fixture(scope="module")
def model_batches(tmp_path_factory):
    """{which: TrainingBatches (wide, B = 5; MaxP: B = 2)} over caches in the small models' vocabulary."""
    from ance_amd.batches import DeviceTokenCache, TrainingBatches
    d = str(tmp_path_factory.mktemp("packed_model"))
    out = {}
    for which, pad, shape, B in (("base_biencoder", 0, (37, 20, 11, 8), 5), ("large_roberta_dot", 1, (37, 20, 11, 8), 5),
                                 ("maxp", 1, (3, 2048, 5, 64), 2)):
        qp, pp = _write_model_caches(d, which, pad, *shape)
        case = "maxp" if which == "maxp" else "small"
        out[which] = TrainingBatches(U.lines_of(case), DeviceTokenCache(qp, DEV), DeviceTokenCache(pp, DEV), B, "msmarco_triplet",
                                     shape[3], shape[1], dtype=torch.long)
    return out


def _run(m, args, autocast):
    from ance_amd import attention as T
    T.dropout_state.to_host(0)
    T.manual_seed(S.SEED)
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        loss = m(*args)[0]
    loss.backward()
    return [loss.detach().clone()] + [q.grad.clone() for q in m.parameters()], T.dropout_state.offsets.get(0, 0)


@pytest.mark.parametrize("precision", ["fp32", "half"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("which", ["base_biencoder", "large_roberta_dot"])
def test_model_on_a_packed_batch_equals_set_packed_rows_on_the_padded_one(model_batches, which, p, precision):
    """The first batch of the pass (it holds empty records) at the "max" capacities: the loss and every parameter gradient bit
    for bit, the same number of draws, the same packed_dropped."""
    tb = model_batches[which]
    m = _model(which, p, precision)
    pb = tb.packed(m)
    Rq, Rb = pb.capacity
    k = 0
    padded, packed = list(tb)[k], list(pb)[k]
    assert int((padded[1].sum(1) == 0).sum() + (padded[4].sum(1) == 0).sum() + (padded[7].sum(1) == 0).sum()) >= 1
    got, draws = _run(m, (packed[0], None, packed[1], None, packed[2], None), precision == "half")
    counted = int(m.packed_dropped)
    m.set_packed_rows(query=Rq, body=Rb)
    m.packed_dropped.zero_()
    want, draws_padded = _run(m, (padded[0], padded[1], padded[3], padded[4], padded[6], padded[7]), precision == "half")
    assert draws == draws_padded and (p == 0.0 or draws > 0)
    assert bool(torch.isfinite(want[0])) and counted == int(m.packed_dropped) == 0
    assert len(got) == len(want) == 1 + len(list(m.parameters()))
    for i, (a, b) in enumerate(zip(got, want)):
        assert _bits_equal(a, b), (i, float((a.double() - b.double()).abs().max()))
    assert any(bool(g.any()) for g in got[1:])


def test_model_counts_the_same_dropped_sequences(model_batches):
    """A body capacity that drops: both paths give a non-finite loss and count the same sequences."""
    tb = model_batches["large_roberta_dot"]
    m = _model("large_roberta_dot", 0.0)
    totals = tb.token_totals()
    Rq, Rb = tb.packed(m).capacity[0], int(min(totals[0, 1:])) - 1   # one row short of the smaller body call: both drop
    assert Rb >= 1
    padded, packed = list(tb)[0], list(tb.packed(m, Rq, Rb))[0]
    with torch.no_grad():
        loss = m(packed[0], None, packed[1], None, packed[2], None)[0]
        counted = int(m.packed_dropped)
        m.set_packed_rows(query=Rq, body=Rb)
        m.packed_dropped.zero_()
        want = m(padded[0], padded[1], padded[3], padded[4], padded[6], padded[7])[0]
    assert counted == int(m.packed_dropped) >= 1 and not bool(torch.isfinite(want)) and _bits_equal(loss, want)


def test_maxp_model_on_packed_chunks(model_batches):
    """RobertaDot_CLF_ANN_NLL_MultiChunk, C = 4 chunks of 512: record 1 has one token, so three of its chunks are all pad."""
    tb = model_batches["maxp"]
    m = _model("maxp", 0.1)
    pb = tb.packed(m)
    assert pb.chunk_len == {"q": 64, "a": 512, "b": 512} and pb.chunks == {"q": 1, "a": 4, "b": 4}
    Rq, Rb = pb.capacity
    padded, packed = list(tb)[0], list(pb)[0]
    assert packed[1].chunks == 4 and packed[1].n_seq == 8
    assert int((packed[1].seq_kept == 0).sum()) + int((packed[2].seq_kept == 0).sum()) >= 1
    got, _ = _run(m, (packed[0], None, packed[1], None, packed[2], None), False)
    m.set_packed_rows(query=Rq, body=Rb)
    want, _ = _run(m, (padded[0], padded[1], padded[3], padded[4], padded[6], padded[7]), False)
    assert bool(torch.isfinite(want[0]))
    for i, (a, b) in enumerate(zip(got, want)):
        assert _bits_equal(a, b), (i, float((a.double() - b.double()).abs().max()))


# ---------------------------------------------------------------------------------------------------------------- capture
def _model_and_optimizer(which, p=0.1):
    from ance_amd import optim
    m = _model(which, p)
    named = list(m.named_parameters())
    groups = [dict(params=[q for n, q in named if S.group_of(n.replace("roberta.", "")) == k], lr=LU.GROUPS[k]["lr"],
                   weight_decay=LU.GROUPS[k]["weight_decay"]) for k in range(len(LU.GROUPS))]
    return m, optim.Lamb(groups, lr=1e-3, betas=LU.BETAS, eps=LU.EPS, max_grad_norm=1.0)


def _snapshot(m, opt):
    return [(q.detach().clone(), opt.state[q]["exp_avg"].clone(), opt.state[q]["exp_avg_sq"].clone()) for q in m.parameters()]


def test_captured_step_with_the_gather_inside_the_graph(model_batches):
    """RobertaDot_NLL_LN + Lamb, dropout 0.1, "max" capacities: ONE graph holds cursor.next(), forward, backward, Lamb.step() and the
    dropout stream's advance; three replays walk three consecutive batches of different totals and equal, in every parameter and
    both moments, three eager host-mode steps fed by iterating the same PackedBatches."""
    from ance_amd import attention as T
    tb, steps = model_batches["large_roberta_dot"], 3
    m, opt = _model_and_optimizer("large_roberta_dot")
    pb = tb.packed(m)
    totals = tb.token_totals()
    assert len({tuple(t) for t in totals[:steps].tolist()}) == steps and len(tb) > steps
    T.dropout_state.to_host(0)
    T.manual_seed(S.SEED)
    want = []
    for t, (q, a, b) in zip(range(steps), pb):
        m(q, None, a, None, b, None)[0].backward()
        opt.step()
        want.append(_snapshot(m, opt))
        opt.zero_grad(set_to_none=True)
    assert int(m.packed_dropped) == 0

    m, opt = _model_and_optimizer("large_roberta_dot")
    pb = tb.packed(m)
    cur = pb.cursor()
    T.dropout_state.to_host(0)
    T.manual_seed(S.SEED)
    T.dropout_state.to_device(0)
    start = [q.detach().clone() for q in m.parameters()]

    def step():
        q, a, b = cur.next()
        m(q, None, a, None, b, None)[0].backward()
        opt.step()
        T.dropout_state.advance(0)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
            opt.zero_grad(set_to_none=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.no_grad():   # back to step 0, in place: no pointer the plan or the graph holds changes
        for q, q0 in zip(m.parameters(), start):
            q.copy_(q0)
            st = opt.state[q]
            st["exp_avg"].zero_()
            st["exp_avg_sq"].zero_()
            if isinstance(st.get("step"), torch.Tensor):
                st["step"].zero_()
    cur.reset()
    T.manual_seed(S.SEED)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    assert int(cur.position) == 0   # the capture ran nothing
    for t in range(steps):
        graph.replay()
        torch.cuda.synchronize()
        assert int(cur.position) == (t + 1) * tb.batch_size
        got = _snapshot(m, opt)
        for (n, _), a, b in zip(m.named_parameters(), want[t], got):
            for k, (x, y) in enumerate(zip(a, b)):
                assert _bits_equal(x, y), "step %d %s %s: max |d| %.3e" % (t, n, "pmv"[k], float((x.double() - y.double()).abs().max()))
    assert int(m.packed_dropped) == 0
    assert not _bits_equal(want[0][0][0], want[1][0][0])
