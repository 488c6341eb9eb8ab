"""The trainers' attention core without a GPU: the restatements the GPU tests lean on, the golden fixture, and every refusal the C ABI
(include/ance_amd.h: ance_attention_*) and the Python wrappers (ance_amd/attention.py) make on the host."""
import ctypes
import json
import os

import numpy as np
import pytest

import attention_train_util as A
from ance_amd import _lib


def _golden(golden_dir):
    with open(os.path.join(golden_dir, "attention_train.json")) as f:
        return json.load(f), np.load(os.path.join(golden_dir, "attention_train.npz"))


def test_philox_known_answers():
    for ctr, key, want in A.PHILOX_KAT:
        got = [int(w) for w in A.philox4x32(*ctr, *key)]
        assert got == list(want), ([hex(g) for g in got], [hex(w) for w in want])


def test_keep_rate_at_p_01():
    """2^20 draws at p = 0.1: the kept fraction is within 5 standard deviations of 0.9."""
    n = 1 << 20
    keep = np.concatenate([A.keep_mask(0.1, 0x123456789abcdef, 7, s, 3, 12, 512, 512).reshape(-1) for s in range(4)])
    assert keep.size == n
    sd = np.sqrt(0.9 * 0.1 / n)
    assert abs(keep.mean() - 0.9) <= 5 * sd, (keep.mean(), sd)
    assert A.keep_threshold(0.1) == int(np.floor(float(np.float32(0.1)) * 2.0 ** 32))
    # word j & 3 of counter word (i * 128 + (j >> 2)) decides key j: one element restated by hand
    w = A.philox4x32(5 * 128 + (9 >> 2), 2 * 12 + 3, 7, 0, 0x89abcdef, 0x1234567)
    assert bool(A.keep_mask(0.1, 0x123456789abcdef, 7, 2, 3, 12, 6, 10)[5, 9]) == bool(int(w[9 & 3]) >= A.keep_threshold(0.1))


def test_golden_fixture_is_the_references(golden_dir):
    """The fixture's recorded facts: the fp64 restatement reproduced the reference's fp64 run (asserted in the generator, <= 1e-12
    relative), and on the committed fp32 inputs the restatement is as far from the reference's fp32 results as the reference's two
    runs are from each other (within the bound's own factor)."""
    meta, g = _golden(golden_dir)
    assert os.path.getsize(os.path.join(golden_dir, "attention_train.npz")) < 774 * 1024
    for case in A.GOLDEN_CASES:
        m = meta[case]
        lens, L = np.asarray(m["lens"]), m["L"]
        assert all(v <= 1e-12 for v in m["fp64_restatement_rel"].values()), m["fp64_restatement_rel"]
        x = {n: A.unpack(g["%s.%s" % (case, n)], lens, L) for n in ("q", "k", "v", "dctx", "ctx", "dq", "dk", "dv")}
        assert x["q"].shape == (len(lens), L, 768) and x["q"].dtype == np.float32
        want = A.attention_fp64(x["q"], x["k"], x["v"], x["dctx"], lens, meta["n_heads"])
        for n in ("ctx", "dq", "dk", "dv"):
            d = float(np.abs(x[n].astype(np.float64) - want[n]).max())
            assert d <= A.bound(m["ref_err"][n], np.abs(want[n]).max()), (case, n, d, m["ref_err"][n])


def test_eager_and_tiled_restatements_agree_with_fp64():
    """The eager fp32 expression and the kernels'-order fp32 restatement against fp64, dropout included, on lengths around the 32-key
    block: the re-ordered evaluation stays within the GPU tests' bound (the measured ratios are printed)."""
    lens, nh = (33, 1, 70, 5), 12
    for p, scale in ((0.0, 1.0), (0.0, 8.0), (0.5, 1.0)):
        q, k, v, g, ln = A.seeded_inputs("cpu.tiles.%g.%g" % (p, scale), lens, nh, q_scale=scale)
        L = q.shape[1]
        keep = A.keep_masks(p, 99, 3, ln, nh, L) if p else None
        want = A.attention_fp64(q, k, v, g, ln, nh, keep, p)
        ref = A.distances(A.eager_fp32(q, k, v, g, ln, nh, keep, p), want)
        got = {n: np.zeros_like(want[n]) for n in A.NAMES}
        for b, n in enumerate(ln):
            for h in range(nh):
                c = slice(64 * h, 64 * h + 64)
                r = A.tiled_fp32(q[b, :, c], k[b, :, c], v[b, :, c], g[b, :, c], int(n), None if keep is None else keep[b, h], p)
                for name, val in zip(("ctx", "dq", "dk", "dv"), (r[0], r[2], r[3], r[4])):
                    got[name][b, :n, c] = val
                got["lse"][h, b * L:b * L + n] = r[1]
        d = A.distances(got, want)
        for n in A.NAMES:
            b_ = A.bound(ref[n], np.abs(want[n]).max())
            print("p %.1f scale %4.1f %-4s tiled %.3e  eager %.3e  ratio %.2f  bound %.3e" % (p, scale, n, d[n], ref[n], d[n] / max(ref[n], 1e-300), b_))
            assert d[n] <= b_, (p, scale, n, d[n], b_)


# ---------------------------------------------------------------------------------------------------------------- C ABI refusals
def _args(**kw):
    fake = 0x10000
    a = _lib.AnceAttnTrainArgs(q=fake, k=fake, v=fake, ctx=fake, ld_q=768, ld_k=768, ld_v=768, ld_ctx=768, d_seq_first=fake,
                               d_seq_len=fake, n_seq=2, max_seq_len=128, n_rows=256, n_heads=12, dropout_p=0.1, training=1, seed=1,
                               offset=0, d_workspace=fake, workspace_bytes=1 << 20)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _grads(**kw):
    fake = 0x10000
    g = _lib.AnceAttnGradArgs(dctx=fake, dq=fake, dk=fake, dv=fake, ld_dctx=768, ld_dq=768, ld_dk=768, ld_dv=768)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def test_workspace_query():
    L = _lib.lib()
    for nh in (12, 16):
        assert L.ance_attention_workspace_bytes(1000, nh) >= 2 * 4 * 1000 * nh
        assert L.ance_attention_workspace_bytes(1, nh) > 0
    # linear in the rows: nothing of size L^2
    assert L.ance_attention_workspace_bytes(8 * 512, 12) <= 2 * 4 * 8 * 512 * 12 + 512
    for nh in (0, 8, 11, 13, 24):
        assert L.ance_attention_workspace_bytes(1000, nh) == 0
    for rows in (0, -1, 1 << 31):
        assert L.ance_attention_workspace_bytes(rows, 12) == 0


def test_c_abi_refuses_before_any_launch():
    """Every refusal of include/ance_amd.h happens on the host: the pointers are fake and never dereferenced."""
    L = _lib.lib()

    def refused(why, fwd_too=True, grads=None, **kw):
        a = _args(**kw)
        g = grads if grads is not None else _grads()
        calls = [("ance_attention_backward", lambda: L.ance_attention_backward(ctypes.byref(a), ctypes.byref(g), None))]
        if fwd_too:
            calls.append(("ance_attention_forward", lambda: L.ance_attention_forward(ctypes.byref(a), None)))
        for fn, call in calls:
            rc, msg = call(), L.ance_last_error().decode()
            assert rc == -1 and fn in msg and why in msg, (fn, why, kw, rc, msg)

    assert L.ance_attention_forward(None, None) == -1
    assert L.ance_attention_backward(None, ctypes.byref(_grads()), None) == -1
    assert L.ance_attention_backward(ctypes.byref(_args()), None, None) == -1 and b"null pointer" in L.ance_last_error()
    for f in ("q", "k", "v", "ctx", "d_seq_first", "d_seq_len"):
        refused("null pointer", **{f: None})
    for nh in (0, 8, 11, 13, 24):
        refused("n_heads", n_heads=nh)
    for m in (0, -1, 513, 1024):
        refused("max_seq_len", max_seq_len=m)
    for n in (0, -3):
        refused("n_seq", n_seq=n)
    refused("n_rows", n_rows=0)
    for r in (-1, 129, 512):
        refused("seq_rows", seq_rows=r)
    for f in ("ld_q", "ld_k", "ld_v", "ld_ctx"):
        for ld in (764, 770, 767, 0, -768):
            refused("stride", **{f: ld})
    refused("stride", n_heads=16)  # the strides of 12 heads
    for f in ("q", "k", "v", "ctx"):
        for off in (4, 8, 2):
            refused("alignment", **{f: 0x10000 + off})
    for p in (-0.1, 1.0, 1.5, float("nan")):
        refused("dropout_p", dropout_p=p)
    refused("workspace", d_workspace=None)
    refused("workspace", d_workspace=0x10000 + 8)
    refused("workspace", workspace_bytes=L.ance_attention_workspace_bytes(256, 12) - 1)
    refused("workspace", workspace_bytes=0)
    for f in ("dctx", "dq", "dk", "dv"):
        refused("null pointer", fwd_too=False, grads=_grads(**{f: None}))
        refused("alignment", fwd_too=False, grads=_grads(**{f: 0x10000 + 4}))
        refused("stride", fwd_too=False, grads=_grads(**{"ld_" + f: 766}))
        refused("stride", fwd_too=False, grads=_grads(**{"ld_" + f: 704}))


# ---------------------------------------------------------------------------------------------------------------- Python wrappers
def test_python_wrappers_refuse_bad_arguments():
    import torch
    from ance_amd import attention as T
    x = torch.zeros(2, 8, 768)
    with pytest.raises(_lib.AnceLibraryError, match="CUDA"):
        T.attention_padded(x, x, x, torch.tensor([8, 3]), 12)
    with pytest.raises(_lib.AnceLibraryError, match="CUDA"):
        T.attention_packed(x[0], x[0], x[0], torch.tensor([0, 8]), 8, 12)
    with pytest.raises(_lib.AnceLibraryError, match="CUDA"):
        T.attention_padded(None, x, x, torch.tensor([8, 3]), 12)
    with pytest.raises(_lib.AnceLibraryError, match=r"\[B, L\]"):
        T.lens_from_mask(torch.ones(8))
    assert T.lens_from_mask(torch.tensor([[1, 1, 0], [1, 0, 0], [0, 0, 0]])).tolist() == [2, 1, 0]
    assert T.lens_from_mask(torch.ones(2, 5)).dtype == torch.int32


def test_python_argument_checks_before_any_device_use():
    """The shape / head / probability checks of _check_inputs, reached with CPU tensors of a torch.Tensor subclass that only claims
    is_cuda.  That works because every check asserted here fires before .device, data_ptr or a launch matters: nothing beyond
    _check_inputs and the length checks in front of the lens / seq_off checks may be reached with these tensors."""
    import torch
    from ance_amd import attention as T

    class Cuda(torch.Tensor):
        is_cuda = True

    def fake(*shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype).as_subclass(Cuda)

    x = fake(2, 8, 768)
    for bad, why in ((dict(n_heads=8), "n_heads"), (dict(n_heads=16), "64 \\* n_heads"), (dict(dropout_p=1.0), "dropout_p"),
                     (dict(dropout_p=-0.5), "dropout_p")):
        kw = dict(dict(n_heads=12, dropout_p=0.0), **bad)
        with pytest.raises(_lib.AnceLibraryError, match=why):
            T._check_inputs(x, x, x, kw["n_heads"], kw["dropout_p"], 3)
    with pytest.raises(_lib.AnceLibraryError, match="float32"):
        T._check_inputs(x, x, fake(2, 8, 768, dtype=torch.float16), 12, 0.0, 3)
    with pytest.raises(_lib.AnceLibraryError, match="one shape"):
        T._check_inputs(x, fake(2, 7, 768), x, 12, 0.0, 3)
    with pytest.raises(_lib.AnceLibraryError, match="3-dimensional"):
        T._check_inputs(fake(8, 768), fake(8, 768), fake(8, 768), 12, 0.0, 3)
    with pytest.raises(_lib.AnceLibraryError, match="1 .. 512"):
        T.attention_padded(fake(1, 513, 768), fake(1, 513, 768), fake(1, 513, 768), None, 12)
    with pytest.raises(_lib.AnceLibraryError, match="max_seq_len"):
        T.attention_packed(fake(8, 768), fake(8, 768), fake(8, 768), None, 0, 12)
    with pytest.raises(_lib.AnceLibraryError, match="seq_off"):
        T.attention_packed(fake(8, 768), fake(8, 768), fake(8, 768), None, 8, 12)


def test_dropout_state_is_a_seeded_call_counter():
    import torch
    from ance_amd import attention as T
    T.manual_seed(1234)
    dev = torch.device("cuda", 0)
    assert [T.dropout_state.next_pair(dev) for _ in range(3)] == [(1234, 0), (1234, 1), (1234, 2)]
    assert T.dropout_state.next_pair(torch.device("cuda", 1)) == (1234, 0)
    T.manual_seed(1234)
    assert T.dropout_state.next_pair(dev) == (1234, 0)
    T.dropout_state.seed = None
    assert T.dropout_state.next_pair(dev)[0] == torch.initial_seed() & 0xFFFFFFFFFFFFFFFF
