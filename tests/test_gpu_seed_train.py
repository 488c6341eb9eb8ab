"""The trainable SEED-Encoder on the GPU (ance_amd.model.SEEDEncoderDot_NLL_LN; ance_pack_tokens_by_id in csrc/pack_rows.hip).
2 layers, hidden 768 throughout.

  1 pack by id        ance_pack_tokens_by_id at its C ABI against ance_amd.packing.pack_tokens (roberta rule) on the torch-compacted
                      batch, EXACTLY: ids, positions, seq_off, seq_kept, dropped, slack rows; guard regions behind every output
  2 leading pads      a sequence that begins with the pad id (an all-pad one too) in mid-batch: dropped, counted, no rows, NaN through
                      the model; its neighbours are those of the batch without it, bit for bit; a PackedTokens under the "seed"
                      rule is run as it is, one under another rule refused
  3 the reference     tests/golden/seed_step.npz, the reference's own SEEDEncoderDot_NLL_LN step in fp64: loss and embeddings 2e-5,
                      every gradient within max(4 x ref_err, 16 ulp32) (train_step_util.compare)
  4 the RoBERTa twin  RobertaDot_NLL_LN with the same weights on the compacted batch at the same capacities: loss and every shared
                      gradient bit for bit, dropout 0.1, fp32 and precision="half" under fp16 / bf16 autocast
  5 replay            one captured step (forward, backward, Lamb) replayed on three batches with different pad patterns
  6 hand-off          Encoder(seed_state_dict(model.reference_state_dict()), ARCH_SEED, fp32) against model.eval().body_emb
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import model_util as M
import seed_util
import train_step_util as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = S.SEED
PAD, VOCAB, MAX_POS = 1, seed_util.SEED_VOCAB, 514
GUARD, SENTINEL = 64, -12345
SRC = seed_util.SRC


@pytest.fixture(autouse=True)
def _host_mode_afterwards():
    from ance_amd import attention as T
    yield
    T.dropout_state.to_host(0)
    T.manual_seed(SEED)


def _np(t):
    return t.detach().float().cpu().numpy()


def _ids(x):
    return torch.from_numpy(np.ascontiguousarray(x)).long().to(DEV)


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).contiguous().view(torch.uint8),
                                                                           b.reshape(-1).contiguous().view(torch.uint8))


def _compact(ids):
    """Every row's non-pad ids moved to the front in their order (a stable sort on "is a pad"), and their counts: on the device."""
    order = torch.sort((ids == PAD).to(torch.int8), dim=1, stable=True).indices
    return ids.gather(1, order), (ids != PAD).sum(1).to(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- 1. pack by id
def _pack_by_id_abi(ids, R, dropped_before=0, vocab=VOCAB, max_pos=MAX_POS):
    """ance_pack_tokens_by_id at its C ABI on sentinel-filled buffers with a guard region behind each; the outputs as NumPy after
    asserting that every guard still holds its sentinel."""
    from ance_amd import _lib
    B, L = ids.shape

    def guarded(n):
        return torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)

    d_ids = ids.to(torch.int32).contiguous()
    lens, off, kept, pid, ppos = guarded(B), guarded(B + 1), guarded(B), guarded(R), guarded(R)
    dropped = torch.full((1 + GUARD,), SENTINEL, dtype=torch.int64, device=DEV)
    dropped[0] = dropped_before
    a = _lib.AncePackByIdArgs(ids=d_ids.data_ptr(), d_seq_len=lens.data_ptr(), d_seq_off=off.data_ptr(), d_seq_kept=kept.data_ptr(),
                              d_dropped=dropped.data_ptr(), packed_ids=pid.data_ptr(), packed_positions=ppos.data_ptr(), n_seq=B, L=L,
                              rows=R, padding_idx=PAD, vocab=vocab, max_pos=max_pos)
    _lib.check(_lib.lib().ance_pack_tokens_by_id(ctypes.byref(a), _lib.current_stream_ptr()), "ance_pack_tokens_by_id")
    torch.cuda.synchronize()
    out = {}
    for name, t, n in (("seq_len", lens, B), ("seq_off", off, B + 1), ("seq_kept", kept, B), ("ids", pid, R), ("positions", ppos, R),
                       ("dropped", dropped, 1)):
        t = t.cpu().numpy()
        assert (t[n:] == SENTINEL).all(), "%s: the guard region behind it was written" % name
        out[name] = t[:n]
    return out


PATTERNS = ("none", "trailing", "interior", "cls_then_pads", "every_second", "outside_vocab", "mixed")


def _pattern_batch(pattern, B, L, seed):
    """ids [B, L] int64 in [3, VOCAB) with pad ids planted by pattern; column 0 is never a pad."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(3, VOCAB, size=(B, L)).astype(np.int64)
    col = np.arange(L)[None, :]
    which = np.full(B, PATTERNS.index(pattern)) if pattern != "mixed" else np.arange(B) % (len(PATTERNS) - 1)
    lens = rng.integers(1, L + 1, size=B)[:, None]
    hit = np.zeros((B, L), bool)
    hit |= (which[:, None] == 1) & (col >= lens)
    hit |= (which[:, None] == 2) & ((col >= lens) | (rng.random((B, L)) < 0.3))
    hit |= (which[:, None] == 3) & (col >= 1)
    hit |= (which[:, None] == 4) & (col % 2 == 1)
    ids[hit & (col >= 1)] = PAD
    out = (which[:, None] == 5) & (rng.random((B, L)) < 0.3)
    ids[out] = np.where(rng.random((B, L)) < 0.5, -7, VOCAB + 11)[out]   # raw ids are kept
    ids[(which[:, None] == 5) & (col >= lens) & (col >= 1)] = PAD
    return ids


@pytest.mark.parametrize("B", [1, 5, 1025])
def test_pack_by_id_equals_pack_tokens_on_the_compacted_batch(B):
    """n_seq 1, 5 and 1,025 (the plan's tile is 1,024 sequences) x L 1, 63, 64, 65, 128, 512 x every pad pattern x R = total,
    total + 5, B * L, total - 1 (the last sequence dropped) and 1."""
    from ance_amd.packing import pack_tokens
    n = 0
    for L in (1, 63, 64, 65, 128, 512):
        for k, pattern in enumerate(PATTERNS):
            if pattern == "mixed" and B < 5:
                continue
            ids = _ids(_pattern_batch(pattern, B, L, 100 * L + k))
            comp, lens = _compact(ids)
            total = int(lens.sum())
            assert total >= B and (pattern != "none" or total == B * L)
            assert L < 63 or B < 5 or pattern == "none" or total < B * L   # the pattern did plant pads
            for R in (total, total + 5, B * L, total - 1, 1):
                if R < 1:
                    continue
                tag = (B, L, pattern, R)
                got = _pack_by_id_abi(ids, R, dropped_before=3)
                counter = torch.full((), 3, dtype=torch.int64, device=DEV)
                want = pack_tokens(comp, lens, R, None, "roberta", PAD, VOCAB, MAX_POS, dropped=counter)
                assert np.array_equal(got["seq_len"], lens.cpu().numpy()), tag
                for name, t in (("seq_off", want.seq_off), ("seq_kept", want.seq_kept), ("ids", want.ids), ("positions", want.positions)):
                    w = t.cpu().numpy()
                    assert np.array_equal(got[name], w), (tag, name, np.nonzero(got[name] != w)[0][:8])
                assert int(got["dropped"][0]) == int(counter), tag
                T = int(got["seq_off"][-1])
                assert (got["ids"][T:] == PAD).all() and (got["positions"][T:] == PAD).all(), tag   # the slack rows
                if R == total - 1:
                    assert got["seq_kept"][-1] == -1 and int(got["dropped"][0]) == 4, tag
                if R >= total:
                    assert int(got["dropped"][0]) == 3 and T == total, tag
                n += 1
    assert n >= 6 * 6 * 4


def test_pack_by_id_clamps_positions_into_a_small_table_and_python_front_end():
    """max_pos below the longest record: the positions clamp as pack_tokens' do; pack_tokens_by_id: "exact" reads the count back,
    an int never synchronises, the caller's counter is added to."""
    from ance_amd.packing import PackRule, pack_tokens, pack_tokens_by_id
    ids = _ids(_pattern_batch("interior", 5, 70, 3))
    comp, lens = _compact(ids)
    total = int(lens.sum())
    got = _pack_by_id_abi(ids, total, max_pos=20)
    want = pack_tokens(comp, lens, total, None, "roberta", PAD, VOCAB, 20)
    assert np.array_equal(got["positions"], want.positions.cpu().numpy()) and got["positions"].max() == 19
    counter = torch.zeros((), dtype=torch.int64, device=DEV)
    for R in ("exact", total + 9, total - 1):
        pk = pack_tokens_by_id(ids, R, PAD, VOCAB, MAX_POS, dropped=counter)
        rows = total if R == "exact" else R
        w = pack_tokens(comp, lens, rows, None, "roberta", PAD, VOCAB, MAX_POS)
        assert pk.rows == rows and pk.max_seq_len == 70 and pk.type_ids is None and pk.dropped is counter and pk.chunks == 1
        assert pk.rule == PackRule.of("seed", PAD, VOCAB, MAX_POS) and pk.rule != w.rule
        for a, b in ((pk.ids, w.ids), (pk.positions, w.positions), (pk.seq_off, w.seq_off), (pk.seq_kept, w.seq_kept)):
            assert torch.equal(a, b), R
    assert int(counter) == 1
    one = pack_tokens_by_id(torch.full((2, 4), PAD, dtype=torch.int64, device=DEV), "exact", PAD)
    assert one.rows == 1 and one.seq_kept.tolist() == [-1, -1] and int(one.dropped) == 2 and one.ids.tolist() == [PAD]


# ---------------------------------------------------------------------------------------------------------------- the models
@functools.lru_cache(maxsize=None)
def _golden(golden_dir):
    with open(os.path.join(golden_dir, "seed_step.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(golden_dir, "seed_step.npz"))


@functools.lru_cache(maxsize=None)
def _weights(golden_dir):
    """(HF names with a zero segment row, the same tensors under the reference's SEED names): the golden step's weights."""
    from oracle import encoder_ref
    meta, _ = _golden(golden_dir)
    w = meta["weights"]
    hf = encoder_ref.det_state_dict(seed=w["seed"], n_layers=w["n_layers"], ln_jitter=w["ln_jitter"], vocab=VOCAB, max_pos=MAX_POS)
    sd = seed_util.to_seed_names(hf)
    assert encoder_ref.state_dict_sha256(sd) == w["checksum"]
    hf = dict(hf)
    hf["roberta.embeddings.token_type_embeddings.weight"] = np.zeros_like(hf["roberta.embeddings.token_type_embeddings.weight"])
    return hf, sd


def _t(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v, np.float32)) for k, v in sd.items()}


def _seed_model(golden_dir, dropout=0.1, precision="fp32"):
    from ance_amd.model import SEEDEncoderDot_NLL_LN
    return SEEDEncoderDot_NLL_LN.from_state_dict(_t(_weights(golden_dir)[1]), precision=precision, dropout=dropout).to(DEV)


def _twin_model(golden_dir, dropout=0.1, precision="fp32"):
    from ance_amd.model import RobertaDot_NLL_LN
    return RobertaDot_NLL_LN.from_state_dict(_t(_weights(golden_dir)[0]), precision=precision, dropout=dropout).to(DEV)


def _golden_args(golden_dir):
    _, g = _golden(golden_dir)
    return [_ids(g["q_ids"]), None, _ids(g["a_ids"]), None, _ids(g["b_ids"]), None]


# ---------------------------------------------------------------------------------------------------------------- 2. leading pads
def test_leading_pad_and_all_pad_sequences_in_mid_batch(golden_dir):
    """Sequence 2 begins with a pad and goes on with tokens, sequence 4 is pads only: both get seq_kept -1, add 1 to dropped each
    and own no rows; seq_off is non-decreasing; the other four have the rows and lengths of the batch without the two.  Through
    the model (eval mode, one capacity for both batches): NaN for the two, packed_dropped counts them, the others' embeddings are
    those of the batch without them, bit for bit."""
    L = 70
    ids = _pattern_batch("interior", 6, L, 11)
    ids[2, 0] = PAD
    ids[2, 1:5] = (5, 6, 7, 8)
    ids[4, :] = PAD
    rest = [0, 1, 3, 5]
    R = 6 * L
    got, base = _pack_by_id_abi(_ids(ids), R), _pack_by_id_abi(_ids(ids[rest]), R)
    assert got["seq_kept"][[2, 4]].tolist() == [-1, -1] and got["seq_len"][[2, 4]].tolist() == [-1, -1]
    assert int(got["dropped"][0]) == 2 and int(base["dropped"][0]) == 0
    assert (np.diff(got["seq_off"]) >= 0).all()
    assert np.array_equal(np.diff(got["seq_off"]), np.where(got["seq_kept"] < 0, 0, got["seq_kept"]))   # they own no rows
    assert np.array_equal(got["seq_kept"][rest], base["seq_kept"]) and np.array_equal(got["seq_off"][rest], base["seq_off"][:-1])
    assert got["seq_off"][-1] == base["seq_off"][-1]
    assert np.array_equal(got["ids"], base["ids"]) and np.array_equal(got["positions"], base["positions"])
    # a leading-pad sequence behind a capacity overflow is an ordinary dropped one: seq_off = T
    short = _pack_by_id_abi(_ids(ids), int(base["seq_off"][1]) + 3)
    assert short["seq_kept"].tolist() == [int(base["seq_kept"][0]), -1, -1, -1, -1, -1] and int(short["dropped"][0]) == 5
    assert short["seq_off"].tolist() == [0] + [int(base["seq_off"][1])] * 6

    m = _seed_model(golden_dir).eval().set_packed_rows(query=R, body=R)
    with torch.no_grad():
        e = m.body_emb(_ids(ids))
        assert int(m.packed_dropped) == 2
        e0 = m.body_emb(_ids(ids[rest]))
        assert int(m.packed_dropped) == 2
    assert torch.isnan(e[[2, 4]]).all() and torch.isfinite(e[rest]).all()
    assert _bits_equal(e[rest], e0)


def test_a_packed_batch_under_the_seed_rule_is_run_as_it_is(golden_dir):
    """body_emb(PackedTokens) equals body_emb(ids) at the same capacity bit for bit and adds the batch's own dropped count; a batch
    packed by length under the roberta rule is refused on the host."""
    from ance_amd import _lib
    from ance_amd.packing import pack_tokens
    ids = _ids(_pattern_batch("interior", 5, 70, 21))
    ids[3, 0] = PAD
    R = 5 * 70
    m = _seed_model(golden_dir).eval().set_packed_rows(body=R)
    tower = m.seed_encoder.encoder.sentence_encoder
    with torch.no_grad():
        want = m.body_emb(ids)
        assert int(m.packed_dropped) == 1
        packed = tower.pack(ids, R)
        got = m.body_emb(packed)
    assert int(m.packed_dropped) == 2 and int(packed.dropped) == 1 and packed.rule == tower.pack_rule
    assert _bits_equal(got, want) and torch.isnan(got[3]).all() and torch.isfinite(got[[0, 1, 2, 4]]).all()
    comp, lens = _compact(ids)
    with pytest.raises(_lib.AnceLibraryError, match="made under"):
        m.body_emb(pack_tokens(comp, lens, R, None, "roberta", PAD, VOCAB, MAX_POS))
    assert int(m.packed_dropped) == 2


# ---------------------------------------------------------------------------------------------------------------- 3. the reference
def test_the_references_own_step(golden_dir):
    """Loss and embeddings within 2e-5 of the reference's fp64 run; every stored gradient within max(4 x ref_err, 16 ulp32), ref_err
    the reference's own fp32 run's distance; k_proj.bias exactly 0; the pad rows of the two tables exactly 0."""
    meta, g = _golden(golden_dir)
    m = _seed_model(golden_dir).eval()
    args = _golden_args(golden_dir)
    loss = m(*args)[0]
    loss.backward()
    with torch.no_grad():
        embs = [m.query_emb(args[0]), m.body_emb(args[2], None), m(args[4], None, is_query=False)]
    assert int(m.packed_dropped) == 0
    for n, e in zip("qab", embs):
        d = float(np.abs(_np(e) - g["emb." + n]).max())
        print("seed step emb %s max|d| %.3e (the reference's own fp32 run: %.3e)" % (n, d, meta["ref_err"]["emb." + n]))
        assert d <= 2e-5, (n, d)
    d = abs(float(loss.detach()) - meta["loss"])
    print("seed step loss %.7f reference %.7f |d| %.3e (the reference's own fp32 run: %.3e)"
          % (float(loss.detach()), meta["loss"], d, meta["ref_err"]["loss"]))
    assert d <= 2e-5, d
    params = dict(m.named_parameters())
    assert list(params) == meta["params"]
    rows = g["rows." + SRC + "embed_tokens.weight"]
    got, want = {}, {}
    for n, p in params.items():
        grad = _np(p.grad).astype(np.float64)
        got[n] = M.golden_view(n, grad[rows] if n == SRC + "embed_tokens.weight" else grad)
        want[n] = g["grad." + n]
        assert got[n].shape == want[n].shape, n
        if n.endswith("self_attn.k_proj.bias"):
            assert not p.grad.any(), n
    bad, worst = S.compare("seed reference step", got, want, meta["ref_err"])
    print("seed reference step largest d / bound %.3f" % worst)
    assert not bad, bad
    assert sum(float(np.abs(want[n]).max()) > 1e-6 for n in params) > len(params) // 2   # not a comparison of zeros
    tokens, positions = params[SRC + "embed_tokens.weight"].grad, params[SRC + "embed_positions.weight"].grad
    assert not tokens[PAD].any() and not positions[PAD].any()
    mask = torch.ones(VOCAB, dtype=torch.bool, device=DEV)
    mask[torch.from_numpy(rows).long().to(DEV)] = False
    assert not tokens[mask].any() and tokens.any() and positions[PAD + 1].any()


# ---------------------------------------------------------------------------------------------------------------- 4. the twin
TWIN_NAMES = [(SRC + "embed_tokens.weight", "roberta.embeddings.word_embeddings.weight"),
              (SRC + "embed_positions.weight", "roberta.embeddings.position_embeddings.weight"),
              (SRC + "emb_layer_norm.weight", "roberta.embeddings.LayerNorm.weight"),
              (SRC + "emb_layer_norm.bias", "roberta.embeddings.LayerNorm.bias")] + \
             [("%slayers.%d.%s.%s" % (SRC, i, fs, t), "roberta.encoder.layer.%d.%s.%s" % (i, hf, t))
              for i in range(2) for hf, fs in seed_util._LAYER for t in ("weight", "bias")] + \
             [(k, k) for k in ("embeddingHead.weight", "embeddingHead.bias", "norm.weight", "norm.bias")]


@pytest.mark.parametrize("dt", ["fp32", "fp16", "bf16"])
def test_roberta_twin_with_dropout_bit_for_bit(golden_dir, dt):
    """The SEED model on the batch with interior pads against RobertaDot_NLL_LN (the same weights under HF names, a zero segment
    row) on the compacted right-padded batch, both at the capacities (Rq, Rb), training mode, dropout 0.1, the same dropout seed
    and offset: the loss and every shared gradient are equal bit for bit."""
    from ance_amd import attention as T
    half = dt != "fp32"
    dtype = dict(fp32=torch.float32, fp16=torch.float16, bf16=torch.bfloat16)[dt]
    args = _golden_args(golden_dir)
    comp = [_compact(x) for x in args[::2]]
    Rq, Rb = int(comp[0][1].sum()) + 3, max(int(comp[1][1].sum()), int(comp[2][1].sum())) + 5
    precision = "half" if half else "fp32"

    def step(m, a):
        T.dropout_state.to_host(0)
        T.manual_seed(SEED)
        with torch.autocast("cuda", dtype=dtype, enabled=half):
            loss = m(*a)[0]
        loss.backward()
        assert int(m.packed_dropped) == 0 and T.dropout_state.offsets[0] == 3 * (1 + 3 * 2)
        return loss.detach(), {n: p.grad for n, p in m.named_parameters()}

    seed = _seed_model(golden_dir, precision=precision).train().set_packed_rows(query=Rq, body=Rb)
    twin = _twin_model(golden_dir, precision=precision).train().set_packed_rows(query=Rq, body=Rb)
    targs = []
    for ids, lens in comp:
        targs += [ids, (torch.arange(ids.shape[1], device=DEV)[None, :] < lens[:, None]).long()]
    ls, gs = step(seed, args)
    lt, gt = step(twin, targs)
    assert torch.isfinite(ls) and _bits_equal(ls, lt), (float(ls), float(lt))
    assert sorted(a for a, _ in TWIN_NAMES) == sorted(gs) and len(gt) == len(gs) + 1   # the twin's segment row is the one extra
    for a, b in TWIN_NAMES:
        assert _bits_equal(gs[a], gt[b]), "%s: max |d| %.3e" % (a, float((gs[a].double() - gt[b].double()).abs().max()))
    assert sum(bool(v.any()) for v in gs.values()) >= len(gs) - 2   # k_proj.bias of the two layers alone is all zeros


# ---------------------------------------------------------------------------------------------------------------- 5. replay
def _replay_inputs(golden_dir, t):
    """The golden step's three batches with another pad pattern at every step t: none beyond the golden ones, every third column,
    a band of pads; column 0 stays."""
    _, g = _golden(golden_dir)
    out = []
    for k, n in enumerate("qab"):
        ids = np.array(g[n + "_ids"])
        col = np.arange(ids.shape[1])[None, :]
        if t == 1:
            ids[np.broadcast_to((col % 3 == 2), ids.shape)] = PAD
        elif t == 2:
            ids[np.broadcast_to((col >= 4 + k) & (col < 9 + 2 * k), ids.shape)] = PAD
        out += [_ids(ids), None]
    return out


def _model_and_optimizer(golden_dir, rows):
    from ance_amd import optim
    m = _seed_model(golden_dir).train().set_packed_rows(query=rows[0], body=rows[1])
    no_decay = ("bias", "LayerNorm.weight")
    named = list(m.named_parameters())
    groups = [dict(params=[p for n, p in named if not any(nd in n for nd in no_decay)], weight_decay=0.01),
              dict(params=[p for n, p in named if any(nd in n for nd in no_decay)], weight_decay=0.0)]
    return m, optim.Lamb(groups, lr=1e-3, eps=1e-6, max_grad_norm=1.0)


def _snapshot(m, opt):
    return [(q.detach().clone(), opt.state[q]["exp_avg"].clone(), opt.state[q]["exp_avg_sq"].clone()) for q in m.parameters()]


def test_one_captured_step_replayed_on_three_pad_patterns(golden_dir):
    """SEEDEncoderDot_NLL_LN + Lamb(max_grad_norm=1.0), dropout 0.1, fixed capacities: one captured step (the pack by id inside
    it), replayed on three batches whose pad patterns and totals differ (fed by copy_), equals three eager host-mode steps in
    every parameter and both moments, bit for bit.  The model, the optimizer and the graph live to the end of the test."""
    from ance_amd import attention as T
    steps = 3
    inputs = [_replay_inputs(golden_dir, t) for t in range(steps)]
    totals = [tuple(int((x != PAD).sum()) for x in a[::2]) for a in inputs]
    assert len(set(totals)) == steps
    rows = (max(t[0] for t in totals) + 2, max(max(t[1:]) for t in totals) + 3)
    m, opt = _model_and_optimizer(golden_dir, rows)
    T.dropout_state.to_host(0)
    T.manual_seed(SEED)
    want = []
    for t in range(steps):
        m(*inputs[t])[0].backward()
        opt.step()
        want.append(_snapshot(m, opt))
        opt.zero_grad(set_to_none=True)
    assert int(m.packed_dropped) == 0
    eager = (m, opt)

    m, opt = _model_and_optimizer(golden_dir, rows)
    T.dropout_state.to_host(0)
    T.manual_seed(SEED)
    T.dropout_state.to_device(0)
    static = [x.clone() if x is not None else None for x in inputs[0]]
    start = [q.detach().clone() for q in m.parameters()]

    def step():
        m(*static)[0].backward()
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
    T.manual_seed(SEED)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for t in range(steps):
        for dst, src in zip(static, inputs[t]):
            if dst is not None:
                dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        got = _snapshot(m, opt)
        for (n, _), a, b in zip(m.named_parameters(), want[t], got):
            for k, (x, y) in enumerate(zip(a, b)):
                assert _bits_equal(x, y), "step %d %s %s: max |d| %.3e" % (t, n, "pmv"[k], float((x.double() - y.double()).abs().max()))
    assert int(m.packed_dropped) == 0
    assert not _bits_equal(want[0][0][0], want[1][0][0])
    assert eager[0] is not None and graph is not None and opt is not None


# ---------------------------------------------------------------------------------------------------------------- 6. hand-off
def test_into_the_encoder(golden_dir):
    """The refresh side: Encoder(seed_state_dict(model.reference_state_dict()), ARCH_SEED, precision="fp32") with no renaming,
    against model.eval().body_emb on the golden passages: 2e-5."""
    from ance_amd.encoder import ARCH_SEED, Encoder, seed_state_dict
    _, g = _golden(golden_dir)
    m = _seed_model(golden_dir).eval()
    enc = Encoder(seed_state_dict(m.reference_state_dict()), ARCH_SEED, "seed.", True, max_seq_len=64, max_tokens=2048, device=DEV,
                  precision="fp32")
    for n in "ab":
        ids = np.ascontiguousarray(g[n + "_ids"], dtype=np.int32)
        lens = (ids.shape[1] - np.argmax(ids[:, ::-1] != PAD, axis=1)).astype(np.int32)   # up to the last non-pad id
        with torch.no_grad():
            want = _np(m.body_emb(_ids(ids)))
        got = enc.encode_ids(torch.from_numpy(ids).to(DEV), torch.from_numpy(lens).to(DEV), h_lens=lens).cpu().numpy()
        d = float(np.abs(got - want).max())
        print("seed hand-off %s max|d| %.3e" % (n, d))
        assert got.shape == want.shape and np.isfinite(got).all() and d <= 2e-5, (n, d)
