"""Packed training batches on the CPU (ance_amd.batches: cum, token_totals, max_token_totals, PackedBatches' refusals): the plan-time
half of the packed gather needs no GPU -- with host TokenCache caches the lengths come from NumPy -- and is checked against the NumPy
restatement of tests/packed_batches_util.py (batches_util's gather composed with packed_util's pack).  All comparisons are exact."""
import ctypes
import random

import numpy as np
import pytest

import batches_util as U
import packed_batches_util as PB
from ance_amd import _lib
from ance_amd.batches import DeviceTokenCache, TrainingBatches, record_lengths
from ance_amd.cache import TokenCache


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("packed_batches"))
    out = {}
    for case in U.CASES:
        qp, pp, lines = U.build_case(case, d)
        out[case] = (TokenCache(qp), TokenCache(pp), lines)
    return out


def make(cases, case, form, world=1, rank=0, batch_size=4):
    qc, pc, lines = cases[case]
    c = U.CASES[case]
    return TrainingBatches(lines, qc, pc, batch_size, form, c["L_q"], c["L_p"], rank=rank, world_size=world)


@pytest.mark.parametrize("case", list(U.CASES))
def test_record_lengths_of_a_host_cache(cases, case):
    """Both rules at chunk_len = L (maxp: 512, four chunks): the header rule spreads min(len, L) over the chunks, the nonzero rule
    counts ids != 0 -- dpr passage 4 has a hole, so the two differ there."""
    _, pc, _ = cases[case]
    L = pc.embedding_size
    ch = min(L, 512)
    C = L // ch
    whole = pc.lengths().astype(np.int64)
    got = record_lengths(pc, ch, _lib.GATHER_MASK_LENGTH).numpy()
    assert got.dtype == np.int32 and got.shape == (len(pc), C) and (got.sum(1) == whole).all()
    for c in range(C):
        assert (got[:, c] == np.clip(whole - c * ch, 0, ch)).all()
    nz = record_lengths(pc, ch, _lib.GATHER_MASK_NONZERO).numpy()
    assert (nz == (pc.ids().reshape(len(pc), C, ch) != 0).sum(2)).all()
    if case == "dpr":
        assert got[4, 0] == 10 and nz[4, 0] == 9
    assert {0, 1, L - 1, L} <= set(whole.tolist()) or len(pc) < 4


@pytest.mark.parametrize("case,form,world,rank", U.combos())
def test_totals_and_max_capacities(cases, case, form, world, rank):
    """cum is the running sum of the restatement's lengths, token_totals() its batch sums, and the "max" totals their maxima, for
    batch sizes 1 / 5 / 64 -- 64 is more than the plan holds: one short batch."""
    qc, pc, _ = cases[case]
    for B in U.BATCH_SIZES:
        random.seed(U.DPR_SEED)
        tb = make(cases, case, form, world, rank, B)
        plan = tb.draw_pass()
        chunk = 512 if case == "maxp" else None
        towers = PB.tower_batches(form, plan, qc, pc, chunk)
        assert tuple(towers) == tb.tower_names()
        for name, (_, lens, C) in towers.items():
            cum = tb.cum(name, chunk).numpy()
            assert cum.dtype == np.int64 and len(cum) == tb.n_items * C + 1
            assert (cum == np.concatenate([[0], np.cumsum(lens)])).all()
        want = PB.batch_totals(towers, tb.n_items, B)
        got = tb.token_totals(chunk)
        assert got.dtype == np.int64 and got.shape == (len(tb), len(towers)) and (got == want).all()
        most = tb.max_token_totals()
        if form.startswith("dpr"):
            assert most == PB.dpr_worst(tb, qc, pc) and (np.array(most) >= want.max(0)).all()
        else:
            assert most == want.max(0).tolist()


@pytest.mark.parametrize("form", U.DPR_FORMS)
def test_dpr_max_holds_for_every_drawn_pass(cases, form):
    """The DPR bound, made before any pass is drawn, against the totals of 20 seeded passes; the totals do change between passes."""
    for B in U.BATCH_SIZES:
        tb = make(cases, "dpr", form, batch_size=B)
        most = np.array(tb.max_token_totals())
        random.seed(U.DPR_SEED)
        seen = set()
        for _ in range(20):
            tb.draw_pass()
            t = tb.token_totals()
            assert (t <= most[None, :]).all(), (B, t.max(0), most)
            seen.add(t.tobytes())
        assert len(seen) > 1


def test_totals_need_a_drawn_pass_for_dpr(cases):
    tb = make(cases, "dpr", "dpr_triplet")
    with pytest.raises(ValueError, match="draw_pass"):
        tb.token_totals()


# ---------------------------------------------------------------------------------------------------------------- refusals
class _NoGpuDeviceCache(DeviceTokenCache):
    """A DeviceTokenCache's host attributes with a device that is never touched: the refusals come before any use of it."""

    def __init__(self, host, device):
        import torch
        self.base_path, self.total_number, self.embedding_size = host.base_path, host.total_number, host.embedding_size
        self.device, self.records = torch.device(device), None


def _cpu_model(pad=0, max_pos=64):
    from ance_amd.model import BiEncoder, TowerConfig
    return BiEncoder(TowerConfig(1000, 768, 1, 3072, max_pos, 2, 1e-12, pad, 0.0, 0.0))


def test_packed_refusals(cases):
    import torch
    from ance_amd.packing import PackedTokens, PackRule
    model = _cpu_model()
    tb = make(cases, "maxp", "msmarco_triplet")
    with pytest.raises(ValueError, match="does not divide"):
        tb.packed(model, chunk_len=500)
    with pytest.raises(ValueError, match="above 512"):
        tb.packed(model, chunk_len=1024)
    with pytest.raises(ValueError, match="above 512"):
        tb.cum("a", 2048)
    with pytest.raises(ValueError, match="query_rows"):
        make(cases, "small", "msmarco_pair").packed(model, query_rows=0)
    with pytest.raises(TypeError, match="DeviceTokenCache"):       # host caches: the plan works, the gather does not
        make(cases, "small", "msmarco_pair").packed(model)
    qc, pc, lines = cases["small"]
    c = U.CASES["small"]
    on_gpu = TrainingBatches(lines, _NoGpuDeviceCache(qc, "cuda:0"), _NoGpuDeviceCache(pc, "cuda:0"), 4, "msmarco_triplet", c["L_q"], c["L_p"])
    with pytest.raises(ValueError, match="the model is on cpu, the token caches on cuda:0"):
        on_gpu.packed(model)
    # a PackedTokens under another rule: refused by the tower, on the host, with both rules in the message
    z = torch.zeros(4, dtype=torch.int32)
    theirs = PackRule.of("roberta", 1, 1000, 64)
    packed = PackedTokens(z, None, z, z[:3], z[:2], 4, 8, torch.zeros((), dtype=torch.int64), theirs)
    for call in (model.query_emb, model.body_emb, lambda p: model(p, None, p, None, p, None)):
        with pytest.raises(_lib.AnceLibraryError) as e:
            call(packed)
        assert "roberta" in str(e.value) and "absolute" in str(e.value)
    assert model.question_model.embeddings.pack_rule == PackRule("absolute", 0, 1000, 64)
    packed.rule = PackRule.of("absolute", 0, 1000, 64)
    with pytest.raises(_lib.AnceLibraryError, match="attention_mask"):
        model.query_emb(packed, z)


FAKE = 0x10000


def _segment(**kw):
    seg = (_lib.AncePackedGatherSegment * 1)()
    s = seg[0]
    s.d_records, s.n_records, s.d_index, s.n_index, s.d_cum = FAKE, 9, FAKE, 20, FAKE
    s.packed_ids, s.packed_positions, s.d_seq_off, s.d_seq_kept, s.d_dropped = FAKE, FAKE, FAKE, FAKE, FAKE
    s.L, s.chunk_len, s.rows, s.position_mode, s.padding_idx, s.vocab, s.max_pos = 2048, 512, 90, 1, 1, 1000, 514
    for k, v in kw.items():
        setattr(s, k, v)
    return seg


def test_the_entry_points_refuse_before_any_launch():
    """The device pointers are fake and never dereferenced: every refusal is made on the host."""
    L = _lib.lib()

    def refused(why, first=0, B=4, d_first=None, n_segs=1, **kw):
        rc, msg = L.ance_gather_batch_packed(_segment(**kw), n_segs, first, B, d_first, None), L.ance_last_error().decode()
        assert rc == -1 and "ance_gather_batch_packed" in msg and why in msg, (why, kw, rc, msg)

    assert L.ance_gather_batch_packed(None, 1, 0, 4, None, None) == -1
    for f in ("d_records", "d_index", "d_cum", "packed_ids", "packed_positions", "d_seq_off", "d_seq_kept", "d_dropped"):
        refused("null pointer", **{f: None})
    for f in ("d_records", "packed_ids", "packed_positions", "d_seq_off", "d_seq_kept"):
        refused("4-byte aligned", **{f: FAKE + 2})
    for f in ("d_index", "d_cum", "d_dropped"):
        refused("8-byte aligned", **{f: FAKE + 4})
    refused("d_first", d_first=FAKE + 4)
    for n in (0, 4):
        refused("n_segs", n_segs=n)
    refused("B < 1", B=0)
    refused("first < 0", first=-1)
    refused("past the item index", first=17)
    refused("past the item index", first=21, B=1)
    refused("chunk_len", chunk_len=0)
    refused("chunk_len", chunk_len=1024)
    refused("does not divide", chunk_len=500)
    refused("65535", B=16384, n_index=1 << 20)
    refused("rows", rows=0)
    refused("n_records", n_records=0)
    refused("empty table", vocab=0)
    refused("empty table", max_pos=0)
    refused("position_mode", position_mode=2)
    refused("padding_idx", padding_idx=-1)
    refused("padding_idx", position_mode=0, padding_idx=-2)
    refused("padding_idx", padding_idx=1000)

    def lengths_refused(why, records=FAKE, n=9, Lr=2048, ch=512, rule=0, out=FAKE):
        rc, msg = L.ance_record_lengths(records, n, Lr, ch, rule, out, None), L.ance_last_error().decode()
        assert rc == -1 and "ance_record_lengths" in msg and why in msg, (why, rc, msg)

    lengths_refused("null pointer", records=None)
    lengths_refused("null pointer", out=None)
    lengths_refused("aligned", records=FAKE + 2)
    lengths_refused("aligned", out=FAKE + 2)
    lengths_refused("n_records", n=0)
    lengths_refused("L < 1", Lr=0)
    lengths_refused("chunk_len", ch=0)
    lengths_refused("chunk_len", Lr=2048, ch=1024)
    lengths_refused("does not divide", ch=500)
    lengths_refused("rule", rule=2)


def test_segment_struct_matches_the_header():
    """The binding's struct against the header's field order and C layout (pointers and int64 first, eight int32 last)."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "ance_amd.h")).read()
    body = re.search(r"typedef struct AncePackedGatherSegment \{(.*?)\} AncePackedGatherSegment;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].replace("void", "").replace("int64_t", "").split(",")]
    names = [n.split()[-1].strip("*") for n in names]
    assert names == [f[0] for f in _lib.AncePackedGatherSegment._fields_]
    assert ctypes.sizeof(_lib.AncePackedGatherSegment) == 10 * 8 + 8 * 4
