"""ance_amd.batches on the CPU: the plan TrainingBatches makes, the random draws of its DPR forms and every refusal, against the
item streams the reference's real loaders produced (tests/golden/batches.npz; generator: tests/golden/make_golden_batches.py, fixture:
tests/batches_util.py).  All comparisons are exact."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

import batches_util as U
from ance_amd import _lib
from ance_amd.batches import TrainingBatches, parse_lines
from ance_amd.cache import TokenCache


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "batches.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(golden_dir, "batches.npz")), meta


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("batches"))
    out = {}
    for case in U.CASES:
        qp, pp, lines = U.build_case(case, d)
        out[case] = (TokenCache(qp), TokenCache(pp), lines)
    return out


def make(cases, case, form, world=1, rank=0, batch_size=4, **kw):
    qc, pc, lines = cases[case]
    c = U.CASES[case]
    kw.setdefault("max_query_length", c["L_q"])
    kw.setdefault("max_seq_length", c["L_p"])
    return TrainingBatches(kw.pop("lines", lines), qc, pc, batch_size, form, rank=rank, world_size=world, **kw)


def test_golden_covers_every_combination(golden):
    arrays, meta = golden
    assert sorted(meta["combos"]) == sorted(U.key(*c) for c in U.combos())
    for c in U.combos():
        assert meta["combos"][U.key(*c)]["arity"] == U.ARITY[c[1]]
    assert meta["dpr_seed"] == U.DPR_SEED


@pytest.mark.parametrize("case,form,world,rank", U.combos())
def test_plan_and_numpy_gather_match_the_reference_loader(golden, cases, case, form, world, rank):
    """.plan equals the record indices the reference's loader read, and a NumPy gather over TokenCache under that plan reproduces
    the loader's tensors in every tuple position (dtypes included)."""
    arrays, meta = golden
    key = U.key(case, form, world, rank)
    random.seed(U.DPR_SEED)
    tb = make(cases, case, form, world, rank)
    plan = tb.draw_pass()
    for col in "qab":
        assert np.array_equal(plan[col], arrays["%s.plan.%s" % (key, col)]), col
    assert tb.n_items == meta["combos"][key]["items"]
    assert len(tb) == -(-tb.n_items // 4)
    got = U.expected_stream(form, plan, cases[case][0], cases[case][1])
    assert len(got) == meta["combos"][key]["arity"]
    for i, x in enumerate(got):
        want = arrays["%s.%d" % (key, i)]
        assert x.dtype == want.dtype and np.array_equal(x, want), (key, i)
    if form == "msmarco_pair":
        assert np.array_equal(plan["label"], arrays[key + ".6"])
    else:
        assert (plan["label"] == -1).all()


@pytest.mark.parametrize("form", U.DPR_FORMS)
@pytest.mark.parametrize("world,rank", U.WORLDS)
def test_dpr_forms_draw_from_random_as_the_reference(golden, cases, form, world, rank):
    """One pass leaves Python's global generator in the state the reference's loader left it in; a second pass draws again and gives
    the reference's second pass; skipped lines draw nothing (the state differs per rank in the golden)."""
    arrays, meta = golden
    key = U.key("dpr", form, world, rank)
    random.seed(U.DPR_SEED)
    tb = make(cases, "dpr", form, world, rank)
    before = random.getstate()
    assert tb.plan is None and random.getstate() == before   # nothing drawn before a pass
    tb.draw_pass()
    state = random.getstate()
    want = meta["random_state_after_one_pass"][key]
    assert state[0] == want[0] and list(state[1]) == want[1] and state[2] == want[2]
    plan2 = tb.draw_pass()
    for col in "qab":
        assert np.array_equal(plan2[col], arrays["%s.pass2.plan.%s" % (key, col)]), col


def test_msmarco_forms_draw_nothing(cases):
    random.seed(3)
    before = random.getstate()
    for form in U.MSMARCO_FORMS:
        tb = make(cases, "small", form)
        assert tb.draw_pass() is tb.plan
    assert random.getstate() == before


def test_lines_from_a_path_and_parse(cases, tmp_path):
    lines = cases["small"][2]
    p = tmp_path / "ann_training_data_0"
    p.write_text("".join(lines))
    a, b = make(cases, "small", "msmarco_triplet", lines=str(p)), make(cases, "small", "msmarco_triplet")
    for col in ("q", "a", "b", "label"):
        assert np.array_equal(a.plan[col], b.plan[col])
    qid, pos, neg, n_neg = parse_lines(["3\t4\t5,6\n", "7\t8\t9"])
    assert qid.tolist() == [3, 7] and pos.tolist() == [4, 8] and neg.tolist() == [5, 6, 9] and n_neg.tolist() == [2, 1]
    for bad in (["3\t4\n"], ["3\t4\t5,\n"], ["3\t4\t5\t6\n"]):
        with pytest.raises(ValueError):
            parse_lines(bad)


def test_plan_time_refusals(cases):
    n_p, n_q = U.CASES["small"]["n_p"], U.CASES["small"]["n_q"]
    msg = "Index {} is out of bound for cached embeddings of size {}"
    for line, key, size in (("0\t1\t-1\n", -1, n_p), ("0\t%d\t1\n" % n_p, n_p, n_p), ("%d\t1\t1\n" % n_q, n_q, n_q),
                            ("-1\t1\t1\n", -1, n_q), ("0\t1\t2,%d\n" % (n_p + 5), n_p + 5, n_p)):
        for form in U.MSMARCO_FORMS:
            with pytest.raises(IndexError) as e:
                make(cases, "small", form, lines=["1\t2\t3\n", line])
            assert str(e.value) == msg.format(key, size)
    with pytest.raises(IndexError):
        make(cases, "dpr", "dpr_triplet", lines=["0\t1\t2,23\n"])
    # the first offender in the reference's reading order: the query of line 0, not the negative of the same line
    with pytest.raises(IndexError) as e:
        make(cases, "small", "msmarco_pair", lines=["%d\t1\t-4\n" % n_q])
    assert str(e.value) == msg.format(n_q, n_q)
    # a bad id on a line another rank reads is not this rank's concern, as in the reference
    make(cases, "small", "msmarco_triplet", world=2, rank=0, lines=["1\t2\t3\n", "0\t1\t-1\n"])
    with pytest.raises(ValueError) as e:
        make(cases, "small", "msmarco_triplet", max_seq_length=128)
    assert "128" in str(e.value) and "20" in str(e.value) and "max_seq_length" in str(e.value)
    with pytest.raises(ValueError) as e:
        make(cases, "small", "msmarco_triplet", max_query_length=64)
    assert "64" in str(e.value) and "8" in str(e.value) and "max_query_length" in str(e.value)
    with pytest.raises(ValueError):
        make(cases, "small", "dpr_pair")                      # DPR reads both caches with one max_seq_length
    with pytest.raises(ValueError) as e:
        make(cases, "small", "msmarco_quadruplet")
    assert "unknown form" in str(e.value)
    for kw in (dict(batch_size=0), dict(world=2, rank=2), dict(world=0)):
        with pytest.raises(ValueError):
            make(cases, "small", "msmarco_triplet", **kw)
    with pytest.raises(TypeError):                            # iteration needs the caches on the device
        next(iter(make(cases, "small", "msmarco_triplet")))


def test_gather_refuses_before_any_launch():
    """Every host-side refusal of ance_gather_batch (include/ance_amd.h) returns ANCE_E_INVALID and names the call; the device
    pointers are fake and never dereferenced."""
    L = _lib.lib()
    fake = 0x10000

    def call(n_segs=2, first=0, B=4, width=_lib.GATHER_REFERENCE, table=True, seg=0, **kw):
        segs = (_lib.AnceGatherSegment * 3)()
        for s in segs:
            s.d_records, s.n_records, s.d_index, s.n_index = fake, 10, fake, 100
            s.d_ids, s.d_mask, s.d_types, s.L = fake, fake, fake, 20
            s.mask_rule, s.type_rule = _lib.GATHER_MASK_LENGTH, _lib.GATHER_TYPES_LENGTH
        for k, v in kw.items():
            setattr(segs[seg], k, v)
        rc = L.ance_gather_batch(segs if table else None, n_segs, first, B, width, None)
        return rc, L.ance_last_error().decode()

    def refused(why, **kw):
        rc, msg = call(**kw)
        assert rc == -1 and "ance_gather_batch" in msg and why in msg, (why, kw, rc, msg)

    refused("null segment table", table=False)
    for seg in (0, 1):
        for field in ("d_records", "d_index", "d_ids", "d_mask"):
            refused("null pointer", seg=seg, **{field: None})
    for n in (-1, 0, 4, 7):
        refused("n_segs", n_segs=n)
    for L_ in (0, -1):
        refused("L < 1", L=L_)
    refused("n_records", n_records=0)
    for B in (0, -3):
        refused("B < 1", B=B)
    refused("first < 0", first=-1)
    refused("past the item index", first=97)
    refused("past the item index", first=101)
    refused("past the item index", B=101)
    refused("past the item index", seg=1, n_index=3)
    for code in (-1, 2, 9):
        refused("unknown mask code", mask_rule=code)
        refused("unknown type code", seg=1, type_rule=code)
        refused("unknown width code", width=code)
    for off in (1, 2, 3):
        refused("d_records not 4-byte aligned", d_records=fake + off)
        for field in ("d_ids", "d_mask", "d_types"):
            refused("aligned", **{field: fake + off})
            refused("aligned", width=_lib.GATHER_WIDE, seg=1, **{field: fake + off})
    refused("aligned", width=_lib.GATHER_WIDE, d_ids=fake + 4)   # int64 outputs: 8-byte
    refused("aligned", d_index=fake + 4)
    # a third segment's fields are not looked at when n_segs = 2 ... and are when it is 3
    refused("L < 1", n_segs=3, seg=2, L=0)
    assert isinstance(ctypes.sizeof(_lib.AnceGatherSegment), int) and ctypes.sizeof(_lib.AnceGatherSegment) == 72
