"""Packed token rows on the CPU: the NumPy restatement of the plan and the packed keys (tests/packed_util.py) checked against
embeddings_util.positions and against its own definition, the mask remapper, and every refusal of the new entry points -- which
happen on the host, before any launch (the device pointers below are fake and never dereferenced)."""
import ctypes

import numpy as np
import pytest

import embeddings_util as E
import layer_tail_util as T
import model_util as M
import packed_util as P
import train_step_util as S
from ance_amd import _lib

VOCAB, MAX_POS = 1000, 514


def _batch(mode, pad, lens, L, seed=5, interior=()):
    ids = E.seeded_ids("packing.%s" % mode, (len(lens), L), (pad or 0) + 1, VOCAB, seed)
    for s, l in interior:
        ids[s, l] = pad
    ids[np.arange(L)[None, :] >= np.asarray(lens)[:, None]] = pad if pad is not None else 0
    return ids


def test_plan_offsets_kept_and_dropped():
    lens, L = (0, 1, 63, 64, 65, 512), 512
    total = sum(lens)
    for R, dropped in ((total, 0), (total + 5, 0), (len(lens) * L, 0), (total - 1, 1), (64, 3), (1, 4)):
        pl = P.plan(lens, L, R)
        assert pl["dropped"] == dropped and pl["T"] <= R
        kept = pl["seq_kept"] >= 0
        assert (pl["seq_kept"][kept] == np.asarray(lens)[kept]).all() and (pl["seq_kept"][~kept] == -1).all()
        assert (pl["seq_off"][:-1][~kept] == pl["T"]).all() and pl["seq_off"][-1] == pl["T"]
        assert (np.diff(pl["seq_off"]) == np.where(kept, lens, 0)).all()   # the differences: what the attention cores take
        assert pl["T"] == int(np.asarray(lens)[kept].sum())
    pl = P.plan((-3, 4 + 7, 2), 4, 100)
    assert pl["seq_kept"].tolist() == [0, 4, 2] and pl["seq_off"].tolist() == [0, 0, 4, 6]


@pytest.mark.parametrize("mode,pad", [("absolute", 0), ("absolute", None), ("roberta", 1)])
def test_packed_positions_are_the_padded_positions(mode, pad):
    lens, L = (0, 1, 63, 64, 65, 70), 70
    interior = ((5, 63), (5, 64), (5, 65), (4, 3)) if mode == "roberta" else ()
    ids = _batch(mode, pad, lens, L, interior=interior)
    total = sum(lens)
    want = E.positions(ids, mode, pad, VOCAB, MAX_POS)
    for R in (total, total + 5):
        pk = P.pack(ids, None, lens, R, mode, pad, VOCAB, MAX_POS)
        back = P.unpack_rows(pk["positions"], pk["seq_off"], pk["seq_kept"], L, -7).reshape(len(lens), L)
        valid = np.arange(L)[None, :] < np.asarray(lens)[:, None]
        assert (back[valid] == want[valid]).all() and (back[~valid] == -7).all()
        assert (P.unpack_rows(pk["ids"], pk["seq_off"], pk["seq_kept"], L, -7).reshape(len(lens), L)[valid] == ids[valid]).all()
        slack = slice(pk["T"], R)
        assert (pk["ids"][slack] == (pad or 0)).all() and (pk["positions"][slack] == (pad if mode == "roberta" else 0)).all()
    if mode == "roberta":   # an interior pad keeps position pad and does not count
        pk = P.pack(ids, None, lens, total, mode, pad, VOCAB, MAX_POS)
        o = pk["seq_off"][5]
        assert pk["positions"][o + 63] == pad and pk["positions"][o + 66] == pad + 64


def test_mask_remapper_and_its_inverse():
    lens, L, H = (3, 0, 5, 1), 6, 8
    pl = P.plan(lens, L, 12)
    packed = np.arange(12 * H).reshape(12, H)
    wide = P.unpack_rows(packed, pl["seq_off"], pl["seq_kept"], L, -1)
    assert wide.shape == (len(lens) * L, H)
    for s, n in enumerate(lens):
        assert (wide[s * L:s * L + n] == packed[pl["seq_off"][s]:pl["seq_off"][s] + n]).all() and (wide[s * L + n:(s + 1) * L] == -1).all()
    assert (P.pack_rows(wide, pl["seq_off"], pl["seq_kept"], L, 12, -1)[:9] == packed[:9]).all()
    # with R = B * L and full sequences the packed masks ARE the padded tower's
    cfg = S.BASE
    full = (4, 4, 4)
    a = P.packed_masks(0.1, S.SEED, 3, cfg, full, 4, 12)
    b = M.first_row_masks(0.1, S.SEED, 3, cfg, full, 4)
    assert (a["embeddings"] == b["embeddings"]).all()
    for x, y in zip(a["layers"], b["layers"]):
        assert all((u == v).all() for u, v in zip(x, y))
    # otherwise row s * L + l carries the R-row call's row off_s + l
    a = P.packed_masks(0.1, S.SEED, 3, cfg, (2, 4, 1), 4, 9)
    small = T.tail_keep_mask(0.1, S.SEED, 3 + 2, 9, cfg["H"])
    assert (a["layers"][0][1][4:8] == small[2:6]).all() and (a["layers"][0][1][8] == small[6]).all() and a["layers"][0][1][2:4].all()


# ---------------------------------------------------------------------------------------------------------------- refusals
FAKE = 0x10000


def _pack_args(**kw):
    a = _lib.AncePackArgs(ids=FAKE, type_ids=None, d_seq_len=FAKE, d_seq_off=FAKE, d_seq_kept=FAKE, d_dropped=FAKE, packed_ids=FAKE,
                          packed_type_ids=None, packed_positions=FAKE, n_seq=3, L=40, rows=90, position_mode=0, padding_idx=0,
                          vocab=VOCAB, max_pos=MAX_POS)
    for k, v in kw.items():
        setattr(a, k, v)
    return ctypes.byref(a)


def test_pack_tokens_refuses_before_any_launch():
    L = _lib.lib()

    def refused(why, **kw):
        rc, msg = L.ance_pack_tokens(_pack_args(**kw), None), L.ance_last_error().decode()
        assert rc == -1 and "ance_pack_tokens" in msg and why in msg, (why, kw, rc, msg)

    assert L.ance_pack_tokens(None, None) == -1
    for f in ("ids", "d_seq_len", "d_seq_off", "d_seq_kept", "d_dropped", "packed_ids", "packed_positions"):
        refused("null pointer", **{f: None})
    refused("null pointer", type_ids=FAKE)                     # types without a place for the packed ones
    for f in ("ids", "d_seq_len", "d_seq_off", "d_seq_kept", "packed_ids", "packed_positions", "type_ids"):
        refused("alignment", **{f: FAKE + 2})
    refused("alignment", d_dropped=FAKE + 4)
    for n in (0, -1, 65536):
        refused("n_seq", n_seq=n)
    for n in (0, -1, 513):
        refused("L outside", L=n)
    for n in (0, -5):
        refused("rows", rows=n)
    for m in (-1, 2, 7):
        refused("position_mode", position_mode=m)
    refused("padding_idx", padding_idx=-2)
    refused("padding_idx", padding_idx=VOCAB)
    refused("padding_idx", position_mode=1, padding_idx=-1)
    refused("empty table", vocab=0)
    refused("empty table", max_pos=0)


def test_first_rows_refuse_before_any_launch():
    L = _lib.lib()

    def args(**kw):
        a = _lib.AnceFirstRowsArgs(rows_matrix=FAKE, first=FAKE, d_seq_off=FAKE, d_seq_kept=FAKE, ld_rows=768, ld_first=768, n_seq=3,
                                   rows=90, H=768, dtype=0)
        for k, v in kw.items():
            setattr(a, k, v)
        return ctypes.byref(a)

    for name in ("ance_first_rows_gather", "ance_first_rows_scatter"):
        fn = getattr(L, name)

        def refused(why, **kw):
            rc, msg = fn(args(**kw), None), L.ance_last_error().decode()
            assert rc == -1 and name in msg and why in msg, (name, why, kw, rc, msg)

        assert fn(None, None) == -1
        for f in ("rows_matrix", "first", "d_seq_off", "d_seq_kept"):
            refused("null pointer", **{f: None})
        refused("alignment", rows_matrix=FAKE + 8)
        refused("alignment", first=FAKE + 4)
        refused("alignment", d_seq_off=FAKE + 2)
        for h in (0, 512, 1000):
            refused("width", H=h)
        for d in (-1, 3):
            refused("dtype", dtype=d)
        for n in (0, 65536):
            refused("n_seq", n_seq=n)
        refused("rows", rows=0)
        refused("stride", ld_rows=764)
        refused("stride", ld_first=770)
        refused("stride", dtype=1, ld_rows=772)                 # a 16-bit row stride is a multiple of 8 elements


def test_embed_rows_refuse_before_any_launch_and_the_padded_form_still_refuses_given_positions():
    L = _lib.lib()

    def args(**kw):
        a = _lib.AnceEmbedArgs(ids=FAKE, type_ids=None, word=FAKE, pos=FAKE, type=FAKE, gamma=FAKE, beta=FAKE, y=FAKE, positions=FAKE,
                               n_seq=90, L=1, H=768, vocab=VOCAB, max_pos=MAX_POS, n_types=2, position_mode=0, padding_idx=0, eps=1e-5,
                               dropout_p=0.0, training=0, seed=0, offset=0, d_workspace=FAKE, workspace_bytes=1 << 30)
        for k, v in kw.items():
            setattr(a, k, v)
        return ctypes.byref(a)

    def refused(why, **kw):
        rc, msg = L.ance_embed_rows_forward(args(**kw), None), L.ance_last_error().decode()
        assert rc == -1 and "ance_embed_rows_forward" in msg and why in msg, (why, kw, rc, msg)

    assert L.ance_embed_rows_forward(None, None) == -1
    refused("L = 1", L=40)
    refused("null pointer", positions=None)
    refused("alignment", positions=FAKE + 2)
    refused("position_mode", position_mode=2)
    refused("padding_idx", position_mode=1, padding_idx=-1)
    refused("width", H=512)
    refused("workspace", workspace_bytes=16)
    g = _lib.AnceEmbedGradArgs(dy=FAKE, dpos=FAKE)              # dpos needs the sorted positions in absolute mode too
    rc = L.ance_embed_rows_backward(args(), ctypes.byref(g), None)
    assert rc == -1 and "pos_keys" in L.ance_last_error().decode()
    assert L.ance_embed_forward(args(L=1, position_mode=2), None) == -1   # ance_embed_forward has no third mode
