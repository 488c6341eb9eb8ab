"""The host side of the replayable training step (no device): the 64-bit offset of the device dropout stream restated, the refusal
of an unaligned stream by every *_dstream entry point, and the dropout state's bookkeeping that needs no GPU."""
import ctypes

import numpy as np
import pytest

from ance_amd import _lib

DSTREAM_CALLS = (("ance_attention", "AnceAttnTrainArgs", "AnceAttnGradArgs"), ("ance_attention16", "AnceAttn16Args", "AnceAttn16GradArgs"),
                 ("ance_layer_tail", "AnceLayerTailArgs", "AnceLayerTailGradArgs"),
                 ("ance_layer_tail16", "AnceLayerTail16Args", "AnceLayerTail16GradArgs"), ("ance_embed", "AnceEmbedArgs", "AnceEmbedGradArgs"))


def split_offset(base, r):
    """(off_lo, off_hi) of the effective offset base + r as the kernels form it: one 64-bit add, wrapping at 2^64, split into the
    two 32-bit counter words -- restated with 32-bit words and an explicit carry."""
    lo = np.uint64(base & 0xFFFFFFFF) + np.uint64(r & 0xFFFFFFFF)
    carry = lo >> np.uint64(32)
    hi = (np.uint64(base >> 32) + np.uint64(r >> 32) + carry) & np.uint64(0xFFFFFFFF)
    return int(lo & np.uint64(0xFFFFFFFF)), int(hi)


@pytest.mark.parametrize("base,r", [(0, 0), (5, 3), (2 ** 32 - 1, 0), (2 ** 32 - 1, 1), (2 ** 32 - 1, 2), (2 ** 32, 2 ** 32 - 1),
                                    (2 ** 63 + 7, 2 ** 33 + 1), (2 ** 64 - 1, 1), (2 ** 64 - 2, 5)])
def test_offset_split_carries_into_the_high_word(base, r):
    off = (base + r) % 2 ** 64
    assert split_offset(base, r) == (off & 0xFFFFFFFF, off >> 32)
    # the host-valued call at (seed, base + r) hands the kernels the same two words: (uint32)offset, (uint32)(offset >> 32)
    assert (int(np.uint64(off).astype(np.uint32)), int((np.uint64(off) >> np.uint64(32)).astype(np.uint32))) == split_offset(base, r)


def test_across_two_to_the_32():
    assert split_offset(2 ** 32 - 1, 0) == (0xFFFFFFFF, 0)
    assert split_offset(2 ** 32 - 1, 1) == (0, 1)
    assert split_offset(2 ** 32 - 1, 2) == (1, 1)


def test_stream_words_are_stored_as_int64_and_read_back_unsigned():
    """The device tensor is int64 (torch has no uint64 arithmetic): a seed or base >= 2^63 is stored as its two's complement and the
    kernels read the same 64 bits."""
    from ance_amd.attention import _as_int64
    for n in (0, 1, 2 ** 63 - 1, 2 ** 63, 0x5EED0123456789AB, 0xFEDCBA9876543210, 2 ** 64 - 1):
        s = _as_int64(n)
        assert -2 ** 63 <= s < 2 ** 63 and s & (2 ** 64 - 1) == n
        assert int(np.array([s], np.int64).view(np.uint64)[0]) == n


def test_every_dstream_entry_point_refuses_an_unaligned_stream_on_the_host():
    """ANCE_E_INVALID before the arguments are looked at and before any launch: the pointers are fake and never dereferenced."""
    L = _lib.lib()
    for stem, args, grads in DSTREAM_CALLS:
        a, g = getattr(_lib, args)(), getattr(_lib, grads)()
        for off in (8, 4, 1):
            bad = ctypes.c_void_p(0x10000 + off)
            assert getattr(L, stem + "_forward_dstream")(ctypes.byref(a), bad, None) == _lib.ANCE_E_INVALID
            assert (stem + "_forward_dstream").encode() in L.ance_last_error() and b"d_stream" in L.ance_last_error()
            assert getattr(L, stem + "_backward_dstream")(ctypes.byref(a), ctypes.byref(g), bad, None) == _lib.ANCE_E_INVALID
            assert (stem + "_backward_dstream").encode() in L.ance_last_error() and b"d_stream" in L.ance_last_error()
    for bad in (None, ctypes.c_void_p(0x10008)):
        assert L.ance_dropout_stream_advance(bad, 1, None) == _lib.ANCE_E_INVALID
        assert b"ance_dropout_stream_advance" in L.ance_last_error()


def test_a_null_stream_is_the_plain_call():
    """The *_dstream sibling with a null stream refuses what the plain entry point refuses, for the plain reason."""
    L = _lib.lib()
    a = _lib.AnceLayerTailArgs()
    assert L.ance_layer_tail_forward(ctypes.byref(a), None) == _lib.ANCE_E_INVALID
    plain = L.ance_last_error().replace(b"ance_layer_tail_forward", b"")
    assert L.ance_layer_tail_forward_dstream(ctypes.byref(a), None, None) == _lib.ANCE_E_INVALID
    assert L.ance_last_error().replace(b"ance_layer_tail_forward_dstream", b"") == plain


def test_host_mode_is_the_default_and_counts_as_before():
    """Nothing changes for code that does not opt in: next_pair hands out (seed, offset) host integers, advance() is a no-op."""
    import torch

    from ance_amd.attention import _DropoutState
    Dev = torch.device("cuda", 0)   # a device with an index: no CUDA call is made for it
    st = _DropoutState()
    st.manual_seed(2 ** 64 + 5)
    assert st.next_pair(Dev) == (5, 0) and st.next_pair(Dev) == (5, 1) and st.offsets == {0: 2}
    st.advance(0)
    assert st.offsets == {0: 2} and st.streams == {} and st.to_host(0) == (5, 2)
    d = st.draw(Dev)
    assert (d.seed, d.offset, d.stream) == (5, 2, None)


# ------------------------------------------------------------------------------------------------------------------ the schedule
def linear_warmup_lr(base_lr, n, warm, total):
    """csrc/lr_schedule.hip restated in NumPy float64: base * lambda(n), lambda(n) = n / max(1, warm) below warm, else
    max(0, (total - n) / max(1, total - warm)) -- two conversions, one division, one max, one product."""
    f = np.float64
    if n < warm:
        lam = f(n) / f(max(1, warm))
    else:
        lam = max(f(0.0), f(total - n) / f(max(1, total - warm)))
    return float(f(base_lr) * lam)


@pytest.mark.parametrize("warm,total,steps", [(2, 5, 8), (0, 3, 5), (3, 3, 5)])
def test_schedule_restatement_is_lambda_lr(warm, total, steps):
    """== on float64 at every step against torch.optim.lr_scheduler.LambdaLR over transformers' lambda, base lrs 1e-6 and 5e-6."""
    import torch
    from transformers import get_linear_schedule_with_warmup
    base = (1e-6, 5e-6)
    sgd = torch.optim.SGD([dict(params=[torch.nn.Parameter(torch.zeros(1))], lr=b) for b in base], lr=1.0)
    sched = get_linear_schedule_with_warmup(sgd, warm, total)
    assert isinstance(sched, torch.optim.lr_scheduler.LambdaLR)
    for n in range(steps + 1):
        assert sched.last_epoch == n
        assert sched.get_last_lr() == [linear_warmup_lr(b, n, warm, total) for b in base], n
        sgd.step()
        sched.step()


def test_plan_entry_points_refuse_on_the_host():
    """The resident plan's host side: sizes, the refusals, and a filled table of the stated size -- no device is touched."""
    L = _lib.lib()
    assert L.ance_lamb_plan_table_bytes(-1, 1, 0) == 0 and L.ance_adamw_plan_table_bytes(1, 0, 0) == 0
    T = (_lib.AnceLambTensor * 2)()
    G = (_lib.AnceLambGroup * 1)()
    for k, numel in enumerate((5, 20000)):
        T[k].p, T[k].g, T[k].m, T[k].v, T[k].numel, T[k].group = 0x1000, 0x2000, 0x3000, 0x4000, numel, 0
    size = L.ance_lamb_plan_table_bytes(2, 1, 20005)
    buf = (ctypes.c_char * size)()
    n_chunks, filled = ctypes.c_int64(-1), ctypes.c_size_t(0)
    args = (buf, size, ctypes.byref(n_chunks), ctypes.byref(filled))
    assert L.ance_lamb_plan_build(T, 2, G, None, 1, *args) == _lib.ANCE_OK
    assert n_chunks.value == 1 + 2 and 0 < filled.value <= size
    assert L.ance_lamb_plan_build(T, 2, G, None, 1, buf, filled.value - 1, ctypes.byref(n_chunks), ctypes.byref(filled)) == _lib.ANCE_E_INVALID
    assert b"ance_lamb_plan_build" in L.ance_last_error() and b"h_tables too small" in L.ance_last_error()
    assert L.ance_lamb_plan_build(None, 2, G, None, 1, *args) == _lib.ANCE_E_INVALID
    T[1].group = 1
    assert L.ance_lamb_plan_build(T, 2, G, None, 1, *args) == _lib.ANCE_E_INVALID and b"group index" in L.ance_last_error()
    for bad in (dict(ws=None), dict(ws=0x10008), dict(ws_bytes=16), dict(mx=-1.0), dict(mx=1.0, norm=None)):
        kw = dict(ws=0x10000, ws_bytes=1 << 20, mx=0.0, norm=0x20000)
        kw.update(bad)
        rc = L.ance_lamb_step_planned(2, 1, 3, 0, kw["mx"], None, None, None, kw["norm"], None, 0x30000, kw["ws"], kw["ws_bytes"], None)
        assert rc == _lib.ANCE_E_INVALID and b"ance_lamb_step_planned" in L.ance_last_error(), bad
        rc = L.ance_adamw_step_planned(2, 1, 3, 1, kw["mx"], None, None, kw["norm"], None, kw["ws"], kw["ws_bytes"], None)
        assert rc == _lib.ANCE_E_INVALID and b"ance_adamw_step_planned" in L.ance_last_error(), bad
    assert L.ance_linear_warmup_step(None, 0x1000, 0x2000, 1, 2, 5, None) == _lib.ANCE_E_INVALID
    assert L.ance_linear_warmup_step(0x1004, 0x1000, 0x2000, 1, 2, 5, None) == _lib.ANCE_E_INVALID

