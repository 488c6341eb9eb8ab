"""The 16-bit BertLayer seams (ance_amd/layers.py precision="half" -> csrc/layer_tail_half.hip) without a GPU: the rounding helper of
tests/layer_half_util.py against torch's own conversion, the fp64 restatement, the six symbols of the C ABI with their host-side
refusals, and the argument checks of the new keyword arguments."""
import ctypes
import os

import numpy as np
import pytest

import layer_half_util as HU
import layer_tail_util as U
from ance_amd import _lib

FAKE = 0x10000
SYMBOLS16 = ("ance_layer_tail16_workspace_bytes", "ance_layer_tail16_forward", "ance_layer_tail16_backward",
             "ance_bias_gelu16_workspace_bytes", "ance_bias_gelu16_forward", "ance_bias_gelu16_backward")


# ---------------------------------------------------------------------------------------------------------------- rounding
def _boundary_values(name):
    mant, emin, emax = HU.FORMATS[name]
    big = (2.0 - 2.0 ** -mant) * 2.0 ** emax
    half_ulp_top = 2.0 ** (emax - mant - 1)
    sub = 2.0 ** (emin - mant)   # the smallest subnormal
    v = [0.0, sub, sub / 2, sub / 2 * (1 + 2.0 ** -20), sub * 1.5, sub * 2.5, sub * 0.49, 2.0 ** emin, 2.0 ** emin * (1 - 2.0 ** -12),
         2.0 ** emin - sub / 2, 1.0, 1.0 + 2.0 ** -(mant + 1), 1.0 + 3 * 2.0 ** -(mant + 1), 1.0 + 2.0 ** -(mant + 1) + 2.0 ** -23,
         2.0 - 2.0 ** -(mant + 1), 2.0 - 2.0 ** -(mant + 2), big, big + half_ulp_top * (1 - 2.0 ** -10), big + half_ulp_top,
         big + half_ulp_top * 1.01, 2.0 * big, 3.0e38, np.inf]
    v = np.asarray(v, np.float64)
    v = v[v <= np.finfo(np.float32).max].tolist() + [np.inf]
    return np.asarray(v + [-t for t in v], np.float32)


@pytest.mark.parametrize("name", HU.DTYPES)
def test_round16_is_torchs_conversion(name):
    import torch
    rng = np.random.default_rng(5)
    wide = (rng.standard_normal(200000) * np.exp2(rng.integers(-30, 18, 200000))).astype(np.float32)   # normals, subnormals, overflow (fp16)
    bits = rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32).view(np.float32)         # any fp32 bit pattern
    bits = bits[~np.isnan(bits)]
    for x in (_boundary_values(name), wide, bits):
        want = torch.from_numpy(x).to(HU.torch_dtype(name)).to(torch.float64).numpy()
        got = HU.round16(x, name)
        assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))
    assert np.isinf(HU.round16(np.float32(65520.0), "fp16")) and HU.round16(np.float32(65519.0), "fp16") == 65504.0   # never clamped
    assert np.isnan(HU.round16(np.float32("nan"), name))


@pytest.mark.parametrize("name", HU.DTYPES)
def test_ulp16(name):
    mant, emin, _ = HU.FORMATS[name]
    x = np.asarray([0.0, 2.0 ** (emin - 3), 2.0 ** emin, 1.0, 1.5, 1.999, 2.0, -3.0, 1000.0])
    want = [2.0 ** (emin - mant)] * 3 + [2.0 ** -mant] * 3 + [2.0 ** (1 - mant)] * 2 + [2.0 ** (9 - mant)]
    assert np.array_equal(HU.ulp16(x, name), np.asarray(want))


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", HU.DTYPES)
def test_restatement_of_the_16_bit_seams(name):
    """On 16-bit-valued x the fp64 seams are layer_tail_util's on g = dy + dy16; the 16-bit outputs are those rounded once, and the
    eager fp32 expression on the same inputs stays within its usual distance (the inputs' width changes nothing in the arithmetic)."""
    x, b, r, g, be, dy = U.tail_inputs("half.cpu", 19, 768)
    x, dy16 = HU.rounded(x, name), HU.rounded(dy * np.float32(0.5), name)
    keep = U.tail_keep_mask(0.1, 7, 3, 19, 768)
    got = HU.tail16_fp64(x, b, r, g, be, 1e-5, dy, dy16, name, keep, 0.1)
    want = U.tail_fp64(x, b, r, g, be, 1e-5, dy.astype(np.float64) + dy16, keep, 0.1)
    for n in U.TAIL_NAMES:
        assert np.array_equal(got[n], want[n]), n
    for n16, n in (("y16", "y"), ("dx16", "dx")):
        assert np.all(np.abs(got[n16] - got[n]) <= 0.5 * HU.ulp16(got[n], name)) and np.array_equal(HU.round16(got[n16], name), got[n16])
    assert np.array_equal(got["dx16"] != 0, keep)   # a dropped element's gradient is exactly 0, a kept one's is not
    only16 = HU.tail16_fp64(x, b, r, g, be, 1e-5, None, dy16, name)
    assert np.array_equal(only16["dbeta"], np.asarray(dy16, np.float64).sum(0))
    eager = U.tail_eager_fp32(x, b, r, g, be, 1e-5, (dy + dy16).astype(np.float32), keep, 0.1)
    ref = U.distances(eager, want, U.TAIL_NAMES)
    for n in U.TAIL_NAMES:
        assert ref[n] <= 64 * 2.0 ** -24 * max(1.0, np.abs(want[n]).max()), (n, ref[n])
    gx, gb, gdy = U.gelu_inputs("half.cpu", 5, 3072)
    gx, gdy = HU.rounded(gx, name), HU.rounded(gdy, name)
    gg = HU.gelu16_fp64(gx, gb, gdy, name)
    ok, worst = HU.within16(gg["y16"], gg["y"], 0.0, name)
    assert ok and worst <= 1.0
    assert not HU.within16(gg["y16"] + 1.01 * HU.ulp16(gg["y16"], name), gg["y"], 0.0, name)[0]


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_lib_declares_the_six_symbols():
    for s in SYMBOLS16:
        assert s in _lib.SYMBOLS, s
    L = _lib.lib()
    for s in SYMBOLS16:
        assert getattr(L, s) is not None
    assert _lib.ABI_VERSION == 7 and L.ance_abi_version() == 7   # only added symbols
    hdr = open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "ance_amd.h")).read()
    for s in SYMBOLS16:
        assert s + "(" in hdr, s
    for struct, fields in ((_lib.AnceLayerTail16Args, ("dtype", "y16", "ld_y16")), (_lib.AnceLayerTail16GradArgs, ("dy16", "ld_dy16")),
                           (_lib.AnceBiasGelu16Args, ("dtype",))):
        names = [f[0] for f in struct._fields_]
        for f in fields:
            assert f in names, (struct, f)
    R = _lib.LAYER_TAIL_ROWS_PER_WORKGROUP
    for n_rows in (1, R - 1, R, R + 1, 2085, 100000):
        for H in (768, 1024):
            assert L.ance_layer_tail16_workspace_bytes(n_rows, H) == L.ance_layer_tail_workspace_bytes(n_rows, H) > 0
        for N in (3072, 4096):
            assert L.ance_bias_gelu16_workspace_bytes(n_rows, N) == L.ance_bias_gelu_workspace_bytes(n_rows, N) > 0
    for rows, w in ((0, 768), (-1, 768), (1 << 31, 768), (100, 512), (100, 3072)):
        assert L.ance_layer_tail16_workspace_bytes(rows, w) == 0
    for rows, w in ((0, 3072), (1 << 31, 4096), (100, 768), (100, 4000)):
        assert L.ance_bias_gelu16_workspace_bytes(rows, w) == 0


def _tail_args(**kw):
    a = _lib.AnceLayerTail16Args(x=FAKE, res=FAKE, bias=FAKE, gamma=FAKE, beta=FAKE, y=FAKE, y16=FAKE, ld_x=768, ld_res=768, ld_y=768,
                                 ld_y16=768, H=768, n_rows=100, dtype=_lib.ANCE_DTYPE_F16, eps=1e-5, dropout_p=0.1, training=1, seed=1,
                                 offset=0, d_workspace=FAKE, workspace_bytes=1 << 22)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _tail_grads(**kw):
    g = _lib.AnceLayerTail16GradArgs(dy=FAKE, dy16=FAKE, dx=FAKE, dres=FAKE, dgamma=FAKE, dbeta=FAKE, dbias=FAKE, ld_dy=768, ld_dy16=768,
                                     ld_dx=768, ld_dres=768)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _gelu_args(**kw):
    a = _lib.AnceBiasGelu16Args(x=FAKE, bias=FAKE, y=FAKE, ld_x=3072, ld_y=3072, N=3072, n_rows=100, dtype=_lib.ANCE_DTYPE_BF16, reserved=0,
                                d_workspace=FAKE, workspace_bytes=1 << 22)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _gelu_grads(**kw):
    g = _lib.AnceBiasGelu16GradArgs(dy=FAKE, dx=FAKE, dbias=FAKE, ld_dy=3072, ld_dx=3072)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


TAIL_REFUSALS = [("width", dict(H=512)), ("width", dict(H=3072)), ("n_rows", dict(n_rows=0)), ("n_rows", dict(n_rows=-5)),
                 ("dtype", dict(dtype=0)), ("dtype", dict(dtype=3)), ("null pointer", dict(x=None)), ("null pointer", dict(res=None)),
                 ("null pointer", dict(gamma=None)), ("alignment", dict(x=FAKE + 8)), ("alignment", dict(x=FAKE + 2)),
                 ("alignment", dict(res=FAKE + 8)), ("alignment", dict(bias=FAKE + 4)), ("alignment", dict(gamma=FAKE + 12)),
                 ("stride", dict(ld_x=772)), ("stride", dict(ld_x=760)), ("stride", dict(ld_res=770)), ("stride", dict(ld_res=0)),
                 ("stride", dict(H=1024)), ("dropout_p", dict(dropout_p=1.0)), ("dropout_p", dict(dropout_p=float("nan"))),
                 ("eps", dict(eps=0.0)), ("workspace", dict(d_workspace=None)), ("workspace", dict(d_workspace=FAKE + 8)),
                 ("workspace", dict(workspace_bytes=0)),
                 # the front end these calls share with the fp32 family: ANCE_DTYPE_F32 (0) stays refused here, after n_rows and
                 # before x; a 16-bit x wants a multiple of 8 (772 passes the fp32 rule), res stays an fp32 matrix
                 ("dtype neither ANCE_DTYPE_F16 nor ANCE_DTYPE_BF16", dict(dtype=0)), ("n_rows < 1", dict(dtype=0, n_rows=0)),
                 ("dtype neither", dict(dtype=0, x=None)), ("dtype neither", dict(dtype=-1)), ("dtype neither", dict(dtype=32)),
                 ("a 16-bit row stride is not a multiple of 8", dict(ld_x=772)), ("stride: not a multiple of 4", dict(ld_res=772 + 2))]
TAIL_FORWARD_ONLY = [("null pointer", dict(y=None)), ("null pointer", dict(beta=None)), ("alignment", dict(y=FAKE + 4)),
                     ("alignment", dict(y16=FAKE + 8)), ("stride", dict(ld_y=766)), ("stride", dict(ld_y16=772))]
TAIL_BAD_GRADS = [("neither dy nor dy16", dict(dy=None, dy16=None)), ("alignment", dict(dy=FAKE + 4)), ("alignment", dict(dy16=FAKE + 8)),
                  ("alignment", dict(dx=FAKE + 8)), ("alignment", dict(dres=FAKE + 4)), ("alignment", dict(dgamma=FAKE + 4)),
                  ("alignment", dict(dbeta=FAKE + 4)), ("alignment", dict(dbias=FAKE + 4)), ("stride", dict(ld_dy=764)),
                  ("stride", dict(ld_dy16=772)), ("stride", dict(ld_dx=772)), ("stride", dict(ld_dres=0))]
GELU_REFUSALS = [("width", dict(N=768)), ("width", dict(N=4000)), ("n_rows", dict(n_rows=0)), ("dtype", dict(dtype=7)),
                 ("null pointer", dict(x=None)), ("null pointer", dict(bias=None)), ("alignment", dict(x=FAKE + 8)),
                 ("alignment", dict(bias=FAKE + 8)), ("stride", dict(ld_x=3076)), ("stride", dict(ld_x=3064)), ("stride", dict(N=4096)),
                 ("dtype neither ANCE_DTYPE_F16 nor ANCE_DTYPE_BF16", dict(dtype=0)), ("n_rows < 1", dict(dtype=0, n_rows=0)),
                 ("dtype neither", dict(dtype=0, x=None)), ("a 16-bit row stride is not a multiple of 8", dict(ld_x=3076))]
GELU_FORWARD_ONLY = [("null pointer", dict(y=None)), ("alignment", dict(y=FAKE + 8)), ("stride", dict(ld_y=3076))]
GELU_BACKWARD_ONLY = [("workspace", dict(d_workspace=None)), ("workspace", dict(d_workspace=FAKE + 4)), ("workspace", dict(workspace_bytes=0))]
GELU_BAD_GRADS = [("null pointer", dict(dy=None)), ("alignment", dict(dy=FAKE + 8)), ("alignment", dict(dx=FAKE + 8)),
                  ("alignment", dict(dbias=FAKE + 4)), ("stride", dict(ld_dy=3076)), ("stride", dict(ld_dx=3000))]


def test_c_abi_refuses_before_any_launch():
    """Every refusal happens on the host: the pointers are fake and never dereferenced."""
    L = _lib.lib()

    def refused(fn, call, why):
        rc, msg = call(), L.ance_last_error().decode()
        assert rc == -1 and fn in msg and why in msg, (fn, why, rc, msg)

    fwd, bwd = "ance_layer_tail16_forward", "ance_layer_tail16_backward"
    for why, kw in TAIL_REFUSALS + TAIL_FORWARD_ONLY:
        refused(fwd, lambda: L.ance_layer_tail16_forward(ctypes.byref(_tail_args(**kw)), None), why)
    for why, kw in TAIL_REFUSALS:
        refused(bwd, lambda: L.ance_layer_tail16_backward(ctypes.byref(_tail_args(**kw)), ctypes.byref(_tail_grads()), None), why)
    for why, kw in TAIL_BAD_GRADS:
        refused(bwd, lambda: L.ance_layer_tail16_backward(ctypes.byref(_tail_args()), ctypes.byref(_tail_grads(**kw)), None), why)
    assert L.ance_layer_tail16_forward(None, None) == -1
    refused(bwd, lambda: L.ance_layer_tail16_backward(ctypes.byref(_tail_args()), None, None), "null pointer")
    full = L.ance_layer_tail16_workspace_bytes(100, 768)
    refused(fwd, lambda: L.ance_layer_tail16_forward(ctypes.byref(_tail_args(workspace_bytes=2 * 512 - 1)), None), "workspace")
    refused(bwd, lambda: L.ance_layer_tail16_backward(ctypes.byref(_tail_args(workspace_bytes=full - 1)), ctypes.byref(_tail_grads()), None),
            "workspace")
    fwd, bwd = "ance_bias_gelu16_forward", "ance_bias_gelu16_backward"
    for why, kw in GELU_REFUSALS + GELU_FORWARD_ONLY:
        refused(fwd, lambda: L.ance_bias_gelu16_forward(ctypes.byref(_gelu_args(**kw)), None), why)
    for why, kw in GELU_REFUSALS + GELU_BACKWARD_ONLY:
        refused(bwd, lambda: L.ance_bias_gelu16_backward(ctypes.byref(_gelu_args(**kw)), ctypes.byref(_gelu_grads()), None), why)
    for why, kw in GELU_BAD_GRADS:
        refused(bwd, lambda: L.ance_bias_gelu16_backward(ctypes.byref(_gelu_args()), ctypes.byref(_gelu_grads(**kw)), None), why)
    refused(bwd, lambda: L.ance_bias_gelu16_backward(ctypes.byref(_gelu_args()), None, None), "null pointer")


# ---------------------------------------------------------------------------------------------------------------- Python
def test_python_checks_of_the_new_keyword_arguments():
    import torch
    from ance_amd import layers as T

    class Cuda(torch.Tensor):   # CPU tensors that only claim is_cuda: every check below fires before a pointer or a launch matters
        is_cuda = True

    def fake(*shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype).as_subclass(Cuda)

    x, x16, v = fake(4, 768), fake(4, 768, dtype=torch.float16), fake(768)
    for bad in ("fp16", "bf16", None, 16):
        with pytest.raises(_lib.AnceLibraryError, match="precision must be"):
            T.dropout_add_layer_norm(x, v, x, v, v, 1e-5, precision=bad)
        with pytest.raises(_lib.AnceLibraryError, match="precision must be"):
            T.bias_gelu(fake(4, 3072), fake(3072), precision=bad)
        with pytest.raises(_lib.AnceLibraryError, match="precision must be"):
            T.BertLayer(768, 12, 3072, precision=bad)
    with pytest.raises(_lib.AnceLibraryError, match="return_half needs"):
        T.dropout_add_layer_norm(x, v, x, v, v, 1e-5, return_half=True)
    with pytest.raises(_lib.AnceLibraryError, match="CUDA"):
        T.dropout_add_layer_norm(torch.zeros(4, 768, dtype=torch.float16), v, x, v, v, 1e-5, precision="half")
    # outside autocast an fp32 x is refused, not cast behind the caller's back
    with pytest.raises(_lib.AnceLibraryError, match="float16 or bfloat16"):
        T.dropout_add_layer_norm(x, v, x, v, v, 1e-5, precision="half")
    with pytest.raises(_lib.AnceLibraryError, match="float16 or bfloat16"):
        T.bias_gelu(fake(4, 3072), fake(3072), precision="half")
    # the residual stream and the parameters stay fp32
    with pytest.raises(_lib.AnceLibraryError, match="residual must have dtype torch.float32"):
        T.dropout_add_layer_norm(x16, v, x16, v, v, 1e-5, precision="half")
    with pytest.raises(_lib.AnceLibraryError, match="weight must have dtype torch.float32"):
        T.dropout_add_layer_norm(x16, v, x, fake(768, dtype=torch.float16), v, 1e-5, precision="half")
    with pytest.raises(_lib.AnceLibraryError, match="bias must have dtype torch.float32"):
        T.bias_gelu(fake(4, 3072, dtype=torch.bfloat16), fake(3072, dtype=torch.bfloat16), precision="half")
    with pytest.raises(_lib.AnceLibraryError, match=r"\[\.\., W\]"):
        T.dropout_add_layer_norm(fake(4, 512, dtype=torch.float16), v, fake(4, 512), v, v, 1e-5, precision="half")
    with pytest.raises(_lib.AnceLibraryError, match="one shape"):
        T.dropout_add_layer_norm(x16, v, fake(5, 768), v, v, 1e-5, precision="half")
    with pytest.raises(_lib.AnceLibraryError, match="dropout_p"):
        T.dropout_add_layer_norm(x16, v, x, v, v, 1e-5, dropout_p=1.0, precision="half")
    # BertLayer: precision="half" implies the half attention; the fp32 layer refuses the half-only arguments; the half layer wants
    # the fp32 residual stream
    assert T.BertLayer(768, 12, 3072, precision="half").attention_precision == "half"
    plain = T.BertLayer(768, 12, 3072)
    assert plain.precision == "fp32" and plain.attention_precision == "fp32"
    assert T.BertLayer(768, 12, 3072, attention_precision="half").precision == "fp32"
    for kw in (dict(return_half=True), dict(hidden_states_half=x16)):
        with pytest.raises(_lib.AnceLibraryError, match="need precision"):
            plain(x, None, **kw)
    half = T.BertLayer(768, 12, 3072, precision="half")
    with pytest.raises(_lib.AnceLibraryError, match="fp32 residual stream"):
        half(fake(1, 4, 768, dtype=torch.float16), None)
    with pytest.raises(_lib.AnceLibraryError, match="float16 or bfloat16"):
        half(fake(1, 4, 768), None)                       # fp32 hidden states outside autocast
    with pytest.raises(_lib.AnceLibraryError, match="hidden_states_half must be"):
        half(fake(1, 4, 768), None, hidden_states_half=fake(1, 4, 768))
