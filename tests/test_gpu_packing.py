"""Packed token rows on the GPU (ance_amd/packing.py, bert_embeddings_packed -> csrc/pack_rows.hip, csrc/embed_train.hip).

  pack kernel      ance_pack_tokens against the NumPy restatement (tests/packed_util.py), EXACTLY: lengths across the wave edge,
                   interior pads, the scan's block edge, every capacity rule, clamped lengths, and a guard region behind every
                   output that no call may touch
  embeddings       bert_embeddings_packed: at dropout 0 the covered rows are the padded call's rows bit for bit; with dropout the
                   mask is the restated one at the PACKED row index; the table gradients are held to embeddings_util.embed_fp64
                   within attention_train_util.bound (4 x the eager fp32 expression's own distance, floor 16 ulp)
  first rows       gather and scatter are exact in the three dtypes; an empty sequence gives zeros and takes no gradient, a dropped
                   one gives NaN
"""
import ctypes

import numpy as np
import pytest
import torch

import embeddings_util as E
import packed_util as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
VOCAB, MAX_POS = 1000, 514
GUARD, SENTINEL = 64, -12345


@pytest.fixture(autouse=True)
def _host_mode_afterwards():
    from ance_amd import attention as T
    yield
    T.dropout_state.to_host(0)
    T.manual_seed(0x5EED0123456789AB)


def _dev(x, dtype=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(DEV)


def _ids(mode, pad, lens, L, seed=5, interior=()):
    ids = E.seeded_ids("gpu_packing.%s" % mode, (len(lens), L), (pad or 0) + 1, VOCAB, seed)
    for s, l in interior:
        ids[s, l] = pad
    ids[np.arange(L)[None, :] >= np.clip(np.asarray(lens), 0, L)[:, None]] = pad if pad is not None else 0
    return ids


def _pack_abi(ids, types, lens, R, mode, pad, dropped_before=0):
    """ance_pack_tokens at its C ABI on buffers with a guard region behind each; returns the outputs as NumPy after asserting that
    every guard still holds its sentinel."""
    from ance_amd import _lib
    B, L = ids.shape

    def guarded(n):
        return torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)

    d_ids, d_lens = _dev(ids), _dev(lens)
    d_types = _dev(types) if types is not None else None
    off, kept, pid, ppos = guarded(B + 1), guarded(B), guarded(R), guarded(R)
    ptt = guarded(R) if types is not None else None
    dropped = torch.full((1 + GUARD,), SENTINEL, dtype=torch.int64, device=DEV)
    dropped[0] = dropped_before
    a = _lib.AncePackArgs(ids=d_ids.data_ptr(), type_ids=d_types.data_ptr() if types is not None else None, d_seq_len=d_lens.data_ptr(),
                          d_seq_off=off.data_ptr(), d_seq_kept=kept.data_ptr(), d_dropped=dropped.data_ptr(), packed_ids=pid.data_ptr(),
                          packed_type_ids=ptt.data_ptr() if types is not None else None, packed_positions=ppos.data_ptr(), n_seq=B, L=L,
                          rows=R, position_mode=_lib.EMBED_POSITION_MODES[mode], padding_idx=-1 if pad is None else pad, vocab=VOCAB,
                          max_pos=MAX_POS)
    _lib.check(_lib.lib().ance_pack_tokens(ctypes.byref(a), _lib.current_stream_ptr()), "ance_pack_tokens")
    torch.cuda.synchronize()
    out = {}
    for name, t, n in (("seq_off", off, B + 1), ("seq_kept", kept, B), ("ids", pid, R), ("positions", ppos, R), ("types", ptt, R),
                       ("dropped", dropped, 1)):
        if t is None:
            out[name] = None
            continue
        t = t.cpu().numpy()
        assert (t[n:] == SENTINEL).all(), "%s: the guard region behind it was written" % name
        out[name] = t[:n]
    return out


def _check_pack(tag, ids, types, lens, R, mode, pad, dropped_before=0):
    got = _pack_abi(ids, types, lens, R, mode, pad, dropped_before)
    want = P.pack(ids, types, lens, R, mode, pad, VOCAB, MAX_POS)
    for n in ("seq_off", "seq_kept", "ids", "positions", "types"):
        if want[n] is None:
            continue
        assert np.array_equal(got[n], want[n]), (tag, n, np.nonzero(got[n] != want[n])[0][:8])
    assert int(got["dropped"][0]) == dropped_before + want["dropped"], (tag, got["dropped"], want["dropped"])
    return got, want


@pytest.mark.parametrize("mode,pad", [("absolute", 0), ("absolute", None), ("roberta", 1)])
def test_pack_kernel_equals_the_restatement_at_every_capacity(mode, pad):
    """Lengths 0, 1, 63, 64, 65 and 512 in one batch; roberta: interior pad ids at columns 63, 64 and 65.  R = total, total + 5,
    n_seq * L, and total - 1 (the last sequence dropped: seq_kept -1, dropped + 1, nothing written at or beyond R)."""
    lens, L = (0, 1, 63, 64, 65, 512), 512
    interior = ((5, 63), (5, 64), (5, 65), (4, 7)) if mode == "roberta" else ()
    ids = _ids(mode, pad, lens, L, interior=interior)
    types = E.seeded_ids("gpu_packing.tt", ids.shape, 0, 2, 5) if mode == "absolute" and pad == 0 else None
    total = sum(lens)
    for R in (total, total + 5, len(lens) * L):
        _, want = _check_pack("R=%d" % R, ids, types, lens, R, mode, pad, dropped_before=3)
        assert want["dropped"] == 0 and want["T"] == total
    got, want = _check_pack("one short", ids, types, lens, total - 1, mode, pad, dropped_before=3)
    assert want["dropped"] == 1 and got["seq_kept"][-1] == -1 and got["seq_off"][-1] == total - 512 == got["seq_off"][-2]
    got, want = _check_pack("R=1", ids, types, lens, 1, mode, pad)
    assert want["dropped"] == 4 and got["seq_kept"].tolist() == [0, 1, -1, -1, -1, -1]


def test_pack_kernel_scan_crosses_its_block_edge_and_a_single_sequence():
    """n_seq = 1, and 1,025 with L = 4: the plan's tile is 1,024 sequences."""
    lens = (np.arange(1025) * 7 + 3) % 5                      # 0 .. 4
    ids = _ids("roberta", 1, lens, 4, seed=9)
    total = int(lens.sum())
    for R in (total, total + 5, 1025 * 4, total - 1, total // 2):
        _check_pack("1025 R=%d" % R, ids, None, lens, R, "roberta", 1)
    one = _ids("absolute", 0, (37,), 40)
    for R in (37, 42, 40, 36):
        got, _ = _check_pack("one R=%d" % R, one, None, (37,), R, "absolute", 0)
    assert got["seq_kept"].tolist() == [-1] and got["seq_off"].tolist() == [0, 0] and int(got["dropped"][0]) == 1


def test_pack_kernel_clamps_lengths_outside_their_range():
    lens, L = (-3, 12 + 7, 5), 12
    ids = E.seeded_ids("gpu_packing.clamp", (3, L), 1, VOCAB, 5)   # no pads: a clamped length reads real columns
    got, _ = _check_pack("clamped", ids, None, lens, 20, "absolute", 0)
    assert got["seq_kept"].tolist() == [0, 12, 5] and got["seq_off"].tolist() == [0, 0, 12, 17]


def test_pack_tokens_python_and_exact_rows():
    from ance_amd.packing import pack_tokens
    lens, L = (12, 0, 5, 1), 12
    ids = _ids("roberta", 1, lens, L)
    counter = torch.zeros((), dtype=torch.int64, device=DEV)
    for R in ("exact", 23, 17):
        pk = pack_tokens(_dev(ids, torch.int64), _dev(lens), R, None, "roberta", 1, VOCAB, MAX_POS, dropped=counter)
        rows = 18 if R == "exact" else R
        want = P.pack(ids, None, lens, rows, "roberta", 1, VOCAB, MAX_POS)
        assert pk.rows == rows and pk.max_seq_len == L and pk.type_ids is None and pk.dropped is counter
        for n, t in (("seq_off", pk.seq_off), ("seq_kept", pk.seq_kept), ("ids", pk.ids), ("positions", pk.positions)):
            assert np.array_equal(t.cpu().numpy(), want[n]), (R, n)
    assert int(counter) == 1                                  # R = 17: the last sequence does not fit
    pk = pack_tokens(_dev(ids), torch.zeros(4, dtype=torch.int32, device=DEV), "exact", None, "roberta", 1)
    assert pk.rows == 1 and pk.ids.tolist() == [1] and int(pk.dropped) == 0   # at least one row


# ---------------------------------------------------------------------------------------------------------------- embeddings
def _tables(H, n_types):
    return E.embed_inputs("gpu_packing.%d" % H, H, VOCAB, MAX_POS, n_types, 61)


def _params(tabs):
    return [torch.from_numpy(np.ascontiguousarray(t)).to(DEV).requires_grad_(True) for t in tabs]


CASES = [("absolute", 0, 768, 2), ("roberta", 1, 768, 1), ("absolute", 0, 1024, 2), ("roberta", 1, 1024, 1)]


@pytest.mark.parametrize("mode,pad,H,n_types", CASES)
def test_packed_embeddings_equal_the_padded_rows_bit_for_bit(mode, pad, H, n_types):
    from ance_amd.embeddings import bert_embeddings, bert_embeddings_packed
    from ance_amd.packing import pack_tokens
    lens, L = (40, 0, 17, 33, 1), 41
    interior = ((0, 3), (3, 20)) if mode == "roberta" else ()
    ids = _ids(mode, pad, lens, L, interior=interior)
    types = E.seeded_ids("gpu_packing.tt2", ids.shape, 0, 2, 5) if n_types == 2 else None
    tabs = _params(_tables(H, n_types))
    d_ids, d_types = _dev(ids, torch.int64), None if types is None else _dev(types, torch.int64)
    with torch.no_grad():
        padded = bert_embeddings(d_ids, *tabs, 1e-5, d_types, mode, pad, 0.0, True).reshape(-1, H)
        for R in (sum(lens), sum(lens) + 5, len(lens) * L):
            pk = pack_tokens(d_ids, _dev(lens), R, d_types, mode, pad, VOCAB, MAX_POS)
            y = bert_embeddings_packed(pk, *tabs, 1e-5, mode, pad, 0.0, True)
            assert y.shape == (R, H) and bool(torch.isfinite(y).all())   # the slack rows too
            pl = P.plan(lens, L, R)
            back = P.unpack_rows(y.cpu().numpy().view(np.uint32), pl["seq_off"], pl["seq_kept"], L, 0)
            valid = (np.arange(L)[None, :] < np.asarray(lens)[:, None]).reshape(-1)
            assert np.array_equal(back[valid], padded.cpu().numpy().view(np.uint32)[valid]), R
            if R > pl["T"]:                                   # a slack row: the embedding of (pad token, type 0, the slack position)
                assert torch.equal(y[pl["T"]], y[R - 1])


def _embed_case(tag, mode, pad, H, n_types, ids, types, lens, R, p, offset_calls=0):
    """The packed call and its backward against embed_fp64 on the padded batch: the keep mask is the R-row call's at the packed row
    index, remapped; dy is zero at pad rows (and at the slack rows of the device call), so the padded statement's table gradients
    are the packed call's."""
    import attention_train_util as A
    from ance_amd import attention as T
    from ance_amd.embeddings import bert_embeddings_packed
    from ance_amd.packing import pack_tokens
    B, L = ids.shape
    tabs_np = _tables(H, n_types)
    tabs = _params(tabs_np)
    pl = P.plan(lens, L, R)
    seed = 0x1234ABCD5678
    T.manual_seed(seed)
    pk = pack_tokens(_dev(ids, torch.int64), _dev(lens), R, None if types is None else _dev(types, torch.int64), mode, pad, VOCAB, MAX_POS)
    y = bert_embeddings_packed(pk, *tabs, 1e-5, mode, pad, p, True)
    dy_packed = np.zeros((R, H), np.float32)                  # zero at the slack rows, as every gradient that reaches them is
    dy_packed[:pl["T"]] = E.embed_dy(tag, pl["T"], H)
    y.backward(torch.from_numpy(dy_packed).to(DEV))
    keep = E.tail_keep_mask(p, seed, 0, R, H) if p > 0 else None
    keep_wide = None if keep is None else P.unpack_rows(keep, pl["seq_off"], pl["seq_kept"], L, True)
    dy_wide = P.unpack_rows(dy_packed, pl["seq_off"], pl["seq_kept"], L, 0)
    args = (ids, types) + tuple(tabs_np) + (1e-5, dy_wide, mode, pad, keep_wide, p)
    want = E.embed_fp64(*args)
    ref = E.distances(E.embed_eager_fp32(*args), want)
    got = dict(y=P.unpack_rows(y.detach().cpu().numpy(), pl["seq_off"], pl["seq_kept"], L, 0), dword=tabs[0].grad.cpu().numpy()[want["word_rows"]],
               dpos=tabs[1].grad.cpu().numpy(), dtype=tabs[2].grad.cpu().numpy(), dgamma=tabs[3].grad.cpu().numpy(),
               dbeta=tabs[4].grad.cpu().numpy())
    valid = (np.arange(L)[None, :] < np.clip(np.asarray(lens), 0, L)[:, None]).reshape(-1)
    want = dict(want, y=np.where(valid[:, None], want["y"], 0))
    if keep is not None:   # the mask itself: a kept element is non-zero, a dropped one an exact zero
        dropped = got["y"][valid] == 0
        assert np.array_equal(dropped, ~keep_wide[valid] | (want["y"][valid] == 0)), tag
    bad = []
    for n in E.NAMES:
        d = float(np.abs(np.asarray(got[n], np.float64) - want[n]).max())
        b = A.bound(ref[n], float(np.abs(want[n]).max()))
        print("%-34s %-6s max|d| %.3e  eager %.3e  ratio %5.2f  bound %.3e" % (tag, n, d, ref[n], d / max(ref[n], 1e-300), b))
        if not d <= b:
            bad.append((n, d, b))
    assert not bad, (tag, bad)
    others = np.setdiff1d(np.arange(VOCAB), want["word_rows"])
    assert not tabs[0].grad.cpu().numpy()[others].any()       # rows that do not occur keep their zeros
    if pad is not None:
        assert not tabs[0].grad[pad].any()
        if mode == "roberta":
            assert not tabs[1].grad[pad].any()


@pytest.mark.parametrize("mode,pad,H,n_types", CASES)
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_packed_embeddings_and_their_gradients_against_fp64(mode, pad, H, n_types, p):
    lens, L = (40, 0, 17, 33, 1), 41
    ids = _ids(mode, pad, lens, L, interior=((0, 3), (3, 20)) if mode == "roberta" else ())
    types = E.seeded_ids("gpu_packing.tt3", ids.shape, 0, 2, 5) if n_types == 2 else None
    R = sum(lens) + (5 if p == 0.1 else 0)
    _embed_case("packed %s %d p=%.1f" % (mode, H, p), mode, pad, H, n_types, ids, types, lens, R, p)


@pytest.mark.parametrize("mode,pad", [("absolute", 0), ("roberta", 1)])
def test_packed_table_gradients_across_the_chunk_edge(mode, pad):
    """Every id equal (one word key of 190 rows: three chunks) and position keys of 65, 64 and 63 rows -- runs that end one past, at and
    one before the 64-row chunk edge of the segmented sum, in packed row order."""
    lens = np.array([3] * 63 + [2, 1])
    ids = np.full((65, 4), 7, np.int64)
    ids[np.arange(4)[None, :] >= lens[:, None]] = pad
    assert [(lens > k).sum() for k in range(3)] == [65, 64, 63]
    _embed_case("chunk edge " + mode, mode, pad, 768, 1, ids, None, lens, int(lens.sum()), 0.0)
    _embed_case("chunk edge slack " + mode, mode, pad, 768, 1, ids, None, lens, int(lens.sum()) + 5, 0.1)


# ---------------------------------------------------------------------------------------------------------------- first rows
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("H", [768, 1024])
def test_first_rows_gather_and_scatter_are_exact(dtype, H):
    from ance_amd.packing import first_rows, pack_tokens
    lens, L = (5, 0, 3, 4), 6
    ids = _ids("absolute", 0, lens, L)
    for R, dropped in ((12, 0), (17, 0), (11, 1)):
        pk = pack_tokens(_dev(ids), _dev(lens), R, None, "absolute", 0)
        x = torch.randn(R, H, device=DEV, generator=torch.Generator(DEV).manual_seed(R)).to(dtype).requires_grad_(True)
        out = first_rows(x, pk)
        assert out.dtype == dtype and out.shape == (4, H)
        assert torch.equal(out[0], x[0].detach()) and torch.equal(out[2], x[5].detach())
        assert not out[1].any()                               # an empty sequence between two kept ones: a zero row
        if dropped:
            assert bool(torch.isnan(out[3]).all()) and int(pk.dropped) == 1
        else:
            assert torch.equal(out[3], x[8].detach())
        g = torch.randn(4, H, device=DEV, generator=torch.Generator(DEV).manual_seed(7)).to(dtype)
        out.backward(g)
        want = torch.zeros(R, H, dtype=dtype, device=DEV)
        want[0], want[5] = g[0], g[2]
        if not dropped:
            want[8] = g[3]
        assert torch.equal(x.grad, want)                      # nothing for the empty and the dropped sequence, zeros everywhere else
