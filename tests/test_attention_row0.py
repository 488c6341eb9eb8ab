"""The first-row attention core without a GPU: the refusals of its C ABI (include/ance_amd.h: ance_attention_row0_*) and its
workspace query.  Every refusal happens on the host, before any launch: the pointers are fake and never dereferenced.  The reasons
are the strings of csrc/attention_common.h (check_args, check_matrix, attention_call) behind common.h's refuse():
"<entry point>: invalid argument (<reason>)", compared whole."""
import ctypes

import pytest

from ance_amd import _lib

FAKE = 0x10000          # a 16-byte aligned address nothing reads
FAKE_STREAM = 0x20000   # an aligned d_stream nothing reads
DTYPES = {"fp32": _lib.ANCE_DTYPE_F32, "fp16": _lib.ANCE_DTYPE_F16, "bf16": _lib.ANCE_DTYPE_BF16}
FWD, FWD_D, BWD, BWD_D = ("ance_attention_row0_forward", "ance_attention_row0_forward_dstream", "ance_attention_row0_backward",
                          "ance_attention_row0_backward_dstream")

NULL = "null pointer"
DTYPE = "dtype not ANCE_DTYPE_F32, _F16 or _BF16"
HEADS = "n_heads not 12 or 16"
MAX_LEN = "max_seq_len outside 1 .. 512"
N_SEQ = "n_seq outside 1 .. 65535"
N_ROWS = "n_rows < 1"
SEQ_ROWS = "seq_rows outside 0 .. max_seq_len"
ALIGN = "alignment: a base is not 16-byte aligned"
STRIDE = "stride: not a multiple of a 16-byte piece or below 64 * n_heads"
DROPOUT = "dropout_p outside [0, 1)"
WS = "null or unaligned workspace"
WS_SMALL = "workspace too small"
D_STREAM = "alignment: d_stream is not 16-byte aligned"


def _align_up(n, a):
    return (n + a - 1) // a * a


def _args(dtype=_lib.ANCE_DTYPE_F32, **kw):
    """Well-formed but for the addresses: 2 sequences of up to 128 rows, 12 heads, the workspace exactly as large as the query says."""
    a = _lib.AnceAttn16Args(q=FAKE, k=FAKE, v=FAKE, ctx=FAKE, ld_q=768, ld_k=768, ld_v=768, ld_ctx=768, d_seq_first=FAKE, d_seq_len=FAKE,
                            n_seq=2, max_seq_len=128, n_rows=256, n_heads=12, seq_rows=128, dtype=dtype, dropout_p=0.1, training=1,
                            seed=1, offset=0, d_workspace=FAKE, workspace_bytes=256)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _grads(**kw):
    g = _lib.AnceAttn16GradArgs(dctx=FAKE, dq=FAKE, dk=FAKE, dv=FAKE, ld_dctx=768, ld_dq=768, ld_dk=768, ld_dv=768)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _calls(a, g, fwd_too=True):
    """(entry point, call) of every entry point the arguments reach; a, g: structs or None."""
    L = _lib.lib()
    pa, pg = (None if a is None else ctypes.byref(a)), (None if g is None else ctypes.byref(g))
    calls = [(BWD, lambda: L.ance_attention_row0_backward(pa, pg, None)),
             (BWD_D, lambda: L.ance_attention_row0_backward_dstream(pa, pg, FAKE_STREAM, None))]
    if fwd_too:
        calls += [(FWD, lambda: L.ance_attention_row0_forward(pa, None)),
                  (FWD_D, lambda: L.ance_attention_row0_forward_dstream(pa, FAKE_STREAM, None))]
    return calls


def _refused(why, a, g, fwd_too=True):
    L = _lib.lib()
    for fn, call in _calls(a, g, fwd_too):
        rc, msg = call(), L.ance_last_error().decode()
        assert rc == _lib.ANCE_E_INVALID and msg == "%s: invalid argument (%s)" % (fn, why), (fn, why, rc, msg)


def _passes_the_argument_check(a):
    """The args are accepted whole: a backward without grads gets past them and is refused for the null grads -- the only null
    pointer in the call.  (A forward that passed would be launched on the fake addresses.)"""
    assert all(getattr(a, f) for f in ("q", "k", "v", "ctx", "d_seq_first", "d_seq_len", "d_workspace"))
    _refused(NULL, a, None, fwd_too=False)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_refusals_before_any_launch(dt):
    d = DTYPES[dt]

    def refused(why, **kw):
        _refused(why, _args(d, **kw), _grads())

    _passes_the_argument_check(_args(d))
    _refused(NULL, None, _grads())          # null args
    _refused(NULL, None, None)
    _refused(NULL, _args(d), None, fwd_too=False)   # null grads
    for f in ("q", "k", "v", "ctx", "d_seq_first", "d_seq_len"):
        refused(NULL, **{f: None})
    for nh in (0, 8, 11, 13, 24):
        refused(HEADS, n_heads=nh)
    for m in (0, -1, 513):
        refused(MAX_LEN, max_seq_len=m)
    for n in (0, -3, 65536):
        refused(N_SEQ, n_seq=n)
    refused(N_ROWS, n_rows=0)
    refused(N_ROWS, n_rows=-5)
    for r in (-1, 129):                     # max_seq_len + 1
        refused(SEQ_ROWS, seq_rows=r)
    for r in (0, 1, 40, 128):               # the packed form and every seq_rows up to max_seq_len pass
        _passes_the_argument_check(_args(d, seq_rows=r))
    for f in ("q", "k", "v", "ctx"):
        for off in (4, 8, 2):
            refused(ALIGN, **{f: FAKE + off})
    for p in (-0.1, 1.0, float("nan")):
        refused(DROPOUT, dropout_p=p)
    _passes_the_argument_check(_args(d, dropout_p=0.0))
    refused(WS, d_workspace=None)
    refused(WS, d_workspace=FAKE + 8)
    refused(WS, d_workspace=FAKE + 4)
    refused(WS_SMALL, workspace_bytes=255)  # one byte short of the two sequences' 256
    for f in ("dctx", "dq", "dk", "dv"):
        _refused(NULL, _args(d), _grads(**{f: None}), fwd_too=False)
        for off in (4, 8, 2):
            _refused(ALIGN, _args(d), _grads(**{f: FAKE + off}), fwd_too=False)
        for ld in (770, 764, 767, 704, 0, -768):
            _refused(STRIDE, _args(d), _grads(**{"ld_" + f: ld}), fwd_too=False)
        if d != _lib.ANCE_DTYPE_F32:
            _refused(STRIDE, _args(d), _grads(**{"ld_" + f: 772}), fwd_too=False)


def test_dtype_set():
    """The three dtypes and nothing else: the 16-bit core's two, plus ANCE_DTYPE_F32 = 0."""
    assert (_lib.ANCE_DTYPE_F32, _lib.ANCE_DTYPE_F16, _lib.ANCE_DTYPE_BF16) == (0, 1, 2)
    for d in (3, -1, 16, 32, 31, 33, 1 << 30, -(1 << 31)):
        _refused(DTYPE, _args(d), _grads())
    for d in (0, 1, 2):
        _passes_the_argument_check(_args(d))


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_stride_rule_per_dtype(dt):
    """A stride is a multiple of the dtype's 16-byte piece (4 fp32, 8 16-bit elements) and at least 64 n_heads.  An accepted stride
    is shown by the refusal that FOLLOWS it in the check (the workspace one byte short), or by none."""
    d = DTYPES[dt]
    fp32 = d == _lib.ANCE_DTYPE_F32
    for f in ("ld_q", "ld_k", "ld_v", "ld_ctx"):
        for ld in (770, 764, 767, 704, 0, -768, 771, 766):   # 764 and 704 are multiples of 4 (704 of 8 too) below 64 * 12
            _refused(STRIDE, _args(d, **{f: ld}), _grads())
        for ld in (776, 784, 3 * 768, 1 << 20):
            _refused(WS_SMALL, _args(d, workspace_bytes=255, **{f: ld}), _grads())
            _passes_the_argument_check(_args(d, **{f: ld}))
        if fp32:                                             # 772 = 4 * 193: a whole number of fp32 pieces, half a 16-bit one
            _refused(WS_SMALL, _args(d, workspace_bytes=255, **{f: 772}), _grads())
            _passes_the_argument_check(_args(d, **{f: 772}))
        else:
            _refused(STRIDE, _args(d, **{f: 772}), _grads())
    _refused(STRIDE, _args(d, n_heads=16), _grads())         # 768: the stride of 12 heads
    _passes_the_argument_check(_args(d, n_heads=16, ld_q=1024, ld_k=1024, ld_v=1024, ld_ctx=1024))


def test_unaligned_d_stream_is_refused_first():
    """d_stream is looked at before anything else: null args, and well-formed ones, with a stream 8 bytes off."""
    L = _lib.lib()
    for a, g in ((None, None), (_args(), _grads())):
        pa, pg = (None if a is None else ctypes.byref(a)), (None if g is None else ctypes.byref(g))
        for off in (8, 4, 1):
            for fn, call in ((FWD_D, lambda: L.ance_attention_row0_forward_dstream(pa, FAKE_STREAM + off, None)),
                             (BWD_D, lambda: L.ance_attention_row0_backward_dstream(pa, pg, FAKE_STREAM + off, None))):
                rc, msg = call(), L.ance_last_error().decode()
                assert rc == _lib.ANCE_E_INVALID and msg == "%s: invalid argument (%s)" % (fn, D_STREAM), (fn, off, rc, msg)


def test_workspace_query_and_extent():
    """(m, l) per (sequence, head): 8 n_seq n_heads bytes rounded up to 256, whatever the row count; the calls ask for exactly that."""
    L = _lib.lib()
    for n_seq in (0, 65536, -1):
        for nh in (12, 16):
            assert L.ance_attention_row0_workspace_bytes(n_seq, nh) == 0, (n_seq, nh)
    for nh in (8, 13, 0, -12):
        assert L.ance_attention_row0_workspace_bytes(5, nh) == 0, nh
    for n_seq in (1, 2, 3, 5, 32, 33, 1000, 65535):
        for nh in (12, 16):
            want = _align_up(8 * n_seq * nh, 256)
            assert L.ance_attention_row0_workspace_bytes(n_seq, nh) == want, (n_seq, nh)
            ld = 64 * nh
            for n_rows in (1, 256, n_seq * 512, 2 ** 31 - 1):   # no row count changes what the calls ask for
                kw = dict(n_seq=n_seq, n_heads=nh, n_rows=n_rows, ld_q=ld, ld_k=ld, ld_v=ld, ld_ctx=ld)
                _passes_the_argument_check(_args(workspace_bytes=want, **kw))
                _refused(WS_SMALL, _args(workspace_bytes=want - 1, **kw), _grads(ld_dctx=ld, ld_dq=ld, ld_dk=ld, ld_dv=ld))
    # the full core's query at the same row count is far larger: a workspace sized for the sequences is what this core takes
    assert L.ance_attention_row0_workspace_bytes(2, 12) == 256 < L.ance_attention_workspace_bytes(256, 12)
