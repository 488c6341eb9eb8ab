"""The BertLayer's row-wise seams without a GPU: the golden fixture, the restatements the GPU tests lean on, the dropout counter, the
module's parameter names and every refusal the C ABI (include/ance_amd.h: ance_layer_tail_*, ance_bias_gelu_*) and the Python
wrappers (ance_amd/layers.py) make on the host."""
import ctypes
import json
import os

import numpy as np
import pytest

import attention_train_util as A
import layer_tail_util as U
from ance_amd import _lib


# ---------------------------------------------------------------------------------------------------------------- fixture
def test_fixture_sizes_and_weights(golden_dir):
    with open(os.path.join(golden_dir, "layer_tail.json")) as f:
        meta = json.load(f)
    with open(os.path.join(golden_dir, "attention_train.json")) as f:
        att = json.load(f)
    for name in list(meta["files"].values()) + ["layer_tail.json"]:
        assert os.path.getsize(os.path.join(golden_dir, name)) < (1 << 20), name
    for case in U.GOLDEN_CASES:
        m = meta[case]
        # the same towers, triplets and weights as the attention fixture
        assert m["weights_sha256"] == att[case]["weights_sha256"] and m["lens"] == att[case]["lens"] and m["L"] == att[case]["L"]
        assert m["n_rows"] == 3 * m["L"]
        for seam in U.TAILS:
            assert m["seams"][seam]["rows"] == m["n_rows"], "the tails commit every row"
        assert 4 <= m["seams"]["intermediate"]["rows"] <= m["n_rows"]
        for seam in U.SEAMS:
            assert all(v <= 1e-12 for v in m["seams"][seam]["fp64_restatement_rel"].values()), (case, seam)


@pytest.mark.parametrize("case", U.GOLDEN_CASES)
def test_restatement_agrees_with_the_references_fp32_tensors(golden_dir, case):
    """On the committed fp32 inputs the fp64 restatement is as far from the reference's fp32 results as the reference's fp32 and
    fp64 runs are from each other (within the bound's own factor); dres is dx in eval mode."""
    m, seams = U.load_golden(golden_dir, case)
    for seam in U.SEAMS:
        t, rec = seams[seam], m["seams"][seam]
        assert t["x"].dtype == np.float32 and t["x"].shape == (rec["rows"], rec["width"])
        want = U.golden_fp64(seam, t, m["eps"])
        for n in U.seam_names(seam):
            d = float(np.abs(t[n].astype(np.float64) - want[n]).max())
            b = U.bound(rec["ref_err"][n], np.abs(want[n]).max())
            print("%-5s %-17s %-6s max|delta| %.3e  ref_err %.3e  bound %.3e" % (case, seam, n, d, rec["ref_err"][n], b))
            assert d <= b, (case, seam, n, d, b)
        if seam in U.TAILS:
            assert np.array_equal(want["dres"], want["dx"])


def test_eager_expressions_agree_with_fp64():
    """The torch fp32 expressions that set the GPU tests' bound against the fp64 restatements, dropout included: float32-sized."""
    x, b, r, g, be, dy = U.tail_inputs("cpu.tail", 37, 768)
    for p in (0.0, 0.5):
        keep = U.tail_keep_mask(p, 11, 3, 37, 768) if p else None
        want = U.tail_fp64(x, b, r, g, be, 1e-5, dy, keep, p)
        d = U.distances(U.tail_eager_fp32(x, b, r, g, be, 1e-5, dy, keep, p), want, U.TAIL_NAMES)
        for n, v in d.items():
            assert v <= 64 * A.ulp32(np.abs(want[n]).max()), (p, n, v)
        if p:
            assert np.all(want["dx"][~keep] == 0) and np.all(want["dx"][keep] != 0)
    assert U.tail_fp64(x, None, r, g, be, 1e-5, dy)["dbias"] is None
    x, b, dy = U.gelu_inputs("cpu.gelu", 9, 3072)
    want = U.gelu_fp64(x, b, dy)
    for n, v in U.distances(U.gelu_eager_fp32(x, b, dy), want, U.GELU_NAMES).items():
        assert v <= 64 * A.ulp32(np.abs(want[n]).max()), (n, v)


def test_layer_composition_matches_torch_autograd_in_double():
    """layer_fp64's hand-written backward against torch's autograd on the same expressions in float64, with all three masks."""
    B, L, H, nh = 2, 5, 768, 12
    lens = np.array([5, 3], np.int32)
    sd = U.layer_weights(H, 3072)
    hs, dout = U.det_normal(3, "cpu.layer.hs", (B, L, H), 1.0), U.det_normal(3, "cpu.layer.dout", (B, L, H), 0.1)
    keeps = (A.keep_masks(0.1, 7, 0, lens, nh, L), U.tail_keep_mask(0.1, 7, 1, B * L, H), U.tail_keep_mask(0.1, 7, 2, B * L, H))
    want = U.layer_fp64(hs, lens, sd, nh, 1e-5, dout, keeps, 0.1, 0.1)
    got = U.layer_torch(hs, lens, sd, nh, 1e-5, dout, keeps, 0.1, 0.1, dtype="float64")
    assert set(U.LAYER_PARAMS) <= set(want) and set(U.LAYER_PARAMS) == set(sd)
    for n in U.LAYER_PARAMS + ("out", "dhs"):
        # attention.self.key.bias has no gradient at all (a softmax does not see a constant added to a row of scores): both sides
        # hold rounding noise there, so the scale is the largest gradient of its kind, not its own
        kind = [k for k in U.LAYER_PARAMS if k.endswith(n.rsplit(".", 1)[-1])] if n in U.LAYER_PARAMS else [n]
        d = float(np.abs(got[n] - want[n]).max() / max(np.abs(want[k]).max() for k in kind))
        assert d <= 1e-11, (n, d)


# ---------------------------------------------------------------------------------------------------------------- the dropout counter
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate(p):
    """2^20 draws of the counter (row, col >> 2, offset lo, offset hi): the kept fraction is within 4 standard deviations of 1 - p."""
    keep = U.tail_keep_mask(p, 0x123456789abcdef, 7, 1024, 1024)
    assert keep.size == 1 << 20
    sd = np.sqrt(p * (1.0 - p) / keep.size)
    assert abs(keep.mean() - (1.0 - p)) <= 4 * sd, (keep.mean(), sd)
    # word col & 3 of the call at (row, col >> 2) decides column col: one element restated by hand, offset above 2^32
    off = (5 << 32) + 9
    w = A.philox4x32(37, 613 >> 2, 9, 5, 0x89abcdef, 0x1234567)
    assert bool(U.tail_keep_mask(p, 0x123456789abcdef, off, 40, 768)[37, 613]) == bool(int(w[613 & 3]) >= A.keep_threshold(p))
    assert U.tail_keep_mask(0.0, 1, 2, 3, 768).all()


# ---------------------------------------------------------------------------------------------------------------- the module
def test_bert_layer_has_the_references_parameter_names(golden_dir):
    import torch
    from ance_amd.layers import BertLayer
    with open(os.path.join(golden_dir, "layer_tail.json")) as f:
        meta = json.load(f)
    for hidden, heads, inter in ((768, 12, 3072), (1024, 16, 4096)):
        layer = BertLayer(hidden, heads, inter, 1e-5, 0.1, 0.1)
        for case in U.GOLDEN_CASES:
            assert list(layer.state_dict().keys()) == meta[case]["layer_param_names"]
        assert [n for n, _ in layer.named_parameters()] == meta["rdot"]["layer_param_names"]
    sd = {k: torch.from_numpy(v) for k, v in U.layer_weights(768, 3072).items()}
    layer = BertLayer(768, 12, 3072, 1e-12, 0.1, 0.1)
    layer.load_state_dict(sd, strict=True)
    assert torch.equal(layer.attention.output.LayerNorm.weight.detach(), sd["attention.output.LayerNorm.weight"])
    assert layer.output.LayerNorm.eps == 1e-12
    for bad in ((512, 8, 2048), (768, 16, 3072), (768, 12, 1024)):
        with pytest.raises(_lib.AnceLibraryError, match="BertLayer"):
            BertLayer(*bad)


def test_python_wrappers_refuse_bad_arguments():
    import torch
    from ance_amd import layers as T
    x, v = torch.zeros(4, 768), torch.zeros(768)
    with pytest.raises(_lib.AnceLibraryError, match="CUDA"):
        T.dropout_add_layer_norm(x, v, x, v, v, 1e-5)
    with pytest.raises(_lib.AnceLibraryError, match="CUDA"):
        T.bias_gelu(torch.zeros(4, 3072), torch.zeros(3072))
    with pytest.raises(_lib.AnceLibraryError, match="CUDA"):
        T.dropout_add_layer_norm(None, v, x, v, v, 1e-5)

    class Cuda(torch.Tensor):   # CPU tensors that only claim is_cuda: every check below fires before a pointer or a launch matters
        is_cuda = True

    def fake(*shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype).as_subclass(Cuda)

    x, v = fake(4, 768), fake(768)
    with pytest.raises(_lib.AnceLibraryError, match="float32"):
        T.dropout_add_layer_norm(fake(4, 768, dtype=torch.float16), v, x, v, v, 1e-5)
    with pytest.raises(_lib.AnceLibraryError, match=r"\[\.\., W\]"):
        T.dropout_add_layer_norm(fake(4, 512), v, fake(4, 512), v, v, 1e-5)
    with pytest.raises(_lib.AnceLibraryError, match=r"\[\.\., W\]"):
        T.bias_gelu(fake(4, 768), v)
    with pytest.raises(_lib.AnceLibraryError, match="one shape"):
        T.dropout_add_layer_norm(x, v, fake(5, 768), v, v, 1e-5)
    with pytest.raises(_lib.AnceLibraryError, match=r"weight must be .*\[768\]"):
        T.dropout_add_layer_norm(x, v, x, fake(1024), v, 1e-5)
    with pytest.raises(_lib.AnceLibraryError, match=r"bias must be .*\[3072\]"):
        T.bias_gelu(fake(4, 3072), v)
    for p in (1.0, -0.5):
        with pytest.raises(_lib.AnceLibraryError, match="dropout_p"):
            T.dropout_add_layer_norm(x, v, x, v, v, 1e-5, dropout_p=p)
    for eps in (0.0, -1e-5):
        with pytest.raises(_lib.AnceLibraryError, match="eps"):
            T.dropout_add_layer_norm(x, v, x, v, v, eps)


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_rows_per_workgroup_and_workspace_queries():
    L = _lib.lib()
    R = _lib.LAYER_TAIL_ROWS_PER_WORKGROUP
    assert L.ance_layer_tail_rows_per_workgroup() == R
    src = open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "ance_amd.h")).read()
    assert "#define ANCE_LAYER_TAIL_ROWS_PER_WORKGROUP %d\n" % R in src
    for n_rows in (1, R - 1, R, R + 1, 4096, 100000):
        n_part, stats = -(-n_rows // R), 2 * (-(-4 * n_rows // 256) * 256)   # a pure function of n_rows
        for H in (768, 1024):
            assert L.ance_layer_tail_workspace_bytes(n_rows, H) == stats + n_part * 3 * H * 4
        for N in (3072, 4096):
            assert L.ance_bias_gelu_workspace_bytes(n_rows, N) == n_part * N * 4
    for w in (0, 512, 767, 3072):
        assert L.ance_layer_tail_workspace_bytes(100, w) == 0
    for w in (0, 768, 1024, 4097):
        assert L.ance_bias_gelu_workspace_bytes(100, w) == 0
    for rows in (0, -1, 1 << 31):
        assert L.ance_layer_tail_workspace_bytes(rows, 768) == 0 and L.ance_bias_gelu_workspace_bytes(rows, 3072) == 0
    assert L.ance_layer_tail_workspace_bytes((1 << 31) - 1, 1024) > 0


FAKE = 0x10000


def tail_args(**kw):
    a = _lib.AnceLayerTailArgs(x=FAKE, res=FAKE, bias=FAKE, gamma=FAKE, beta=FAKE, y=FAKE, ld_x=768, ld_res=768, ld_y=768, H=768,
                               n_rows=100, eps=1e-5, dropout_p=0.1, training=1, seed=1, offset=0, d_workspace=FAKE, workspace_bytes=1 << 22)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def tail_grads(**kw):
    g = _lib.AnceLayerTailGradArgs(dy=FAKE, dx=FAKE, dres=FAKE, dgamma=FAKE, dbeta=FAKE, dbias=FAKE, ld_dy=768, ld_dx=768, ld_dres=768)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def gelu_args(**kw):
    a = _lib.AnceBiasGeluArgs(x=FAKE, bias=FAKE, y=FAKE, ld_x=3072, ld_y=3072, N=3072, n_rows=100, d_workspace=FAKE, workspace_bytes=1 << 22)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def gelu_grads(**kw):
    g = _lib.AnceBiasGeluGradArgs(dy=FAKE, dx=FAKE, dbias=FAKE, ld_dy=3072, ld_dx=3072)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


# (why, field changes): what both calls of a pair refuse; TAIL_FORWARD_ONLY / GELU_FORWARD_ONLY: fields the backward does not read
TAIL_REFUSALS = [("width", dict(H=512)), ("width", dict(H=3072)), ("width", dict(H=0)), ("n_rows", dict(n_rows=0)), ("n_rows", dict(n_rows=-5)),
                 ("null pointer", dict(x=None)), ("null pointer", dict(res=None)), ("null pointer", dict(gamma=None)),
                 ("alignment", dict(x=FAKE + 4)), ("alignment", dict(res=FAKE + 8)), ("alignment", dict(bias=FAKE + 4)),
                 ("alignment", dict(gamma=FAKE + 12)), ("stride", dict(ld_x=764)), ("stride", dict(ld_x=770)), ("stride", dict(ld_res=0)),
                 ("stride", dict(ld_res=-768)), ("stride", dict(H=1024)), ("dropout_p", dict(dropout_p=1.0)), ("dropout_p", dict(dropout_p=-0.1)),
                 ("dropout_p", dict(dropout_p=float("nan"))), ("eps", dict(eps=0.0)), ("eps", dict(eps=-1e-5)), ("eps", dict(eps=float("nan"))),
                 ("workspace", dict(d_workspace=None)), ("workspace", dict(d_workspace=FAKE + 8)), ("workspace", dict(workspace_bytes=0))]
TAIL_FORWARD_ONLY = [("null pointer", dict(y=None)), ("null pointer", dict(beta=None)), ("alignment", dict(y=FAKE + 4)),
                     ("alignment", dict(beta=FAKE + 4)), ("stride", dict(ld_y=766))]
GELU_REFUSALS = [("width", dict(N=768)), ("width", dict(N=4000)), ("n_rows", dict(n_rows=0)), ("null pointer", dict(x=None)),
                 ("null pointer", dict(bias=None)), ("alignment", dict(x=FAKE + 4)), ("alignment", dict(bias=FAKE + 8)),
                 ("stride", dict(ld_x=3070)), ("stride", dict(ld_x=3068)), ("stride", dict(N=4096))]
GELU_FORWARD_ONLY = [("null pointer", dict(y=None)), ("alignment", dict(y=FAKE + 4)), ("stride", dict(ld_y=3000))]
GELU_BACKWARD_ONLY = [("workspace", dict(d_workspace=None)), ("workspace", dict(d_workspace=FAKE + 4)), ("workspace", dict(workspace_bytes=0))]


def test_c_abi_refuses_before_any_launch():
    """Every refusal of include/ance_amd.h happens on the host: the pointers are fake and never dereferenced."""
    L = _lib.lib()

    def refused(fn, call, why):
        rc, msg = call(), L.ance_last_error().decode()
        assert rc == -1 and fn in msg and why in msg, (fn, why, rc, msg)

    fwd, bwd = "ance_layer_tail_forward", "ance_layer_tail_backward"
    for why, kw in TAIL_REFUSALS + TAIL_FORWARD_ONLY:
        refused(fwd, lambda: L.ance_layer_tail_forward(ctypes.byref(tail_args(**kw)), None), why)
    for why, kw in TAIL_REFUSALS:
        refused(bwd, lambda: L.ance_layer_tail_backward(ctypes.byref(tail_args(**kw)), ctypes.byref(tail_grads()), None), why)
    assert L.ance_layer_tail_forward(None, None) == -1
    assert L.ance_layer_tail_backward(None, ctypes.byref(tail_grads()), None) == -1
    refused(bwd, lambda: L.ance_layer_tail_backward(ctypes.byref(tail_args()), None, None), "null pointer")
    # the forward needs the statistics only, the backward the partial rows as well
    stats, full = 2 * 512, L.ance_layer_tail_workspace_bytes(100, 768)
    refused(fwd, lambda: L.ance_layer_tail_forward(ctypes.byref(tail_args(workspace_bytes=stats - 1)), None), "workspace")
    refused(bwd, lambda: L.ance_layer_tail_backward(ctypes.byref(tail_args(workspace_bytes=full - 1)), ctypes.byref(tail_grads()), None), "workspace")
    for why, kw in (("null pointer", dict(dy=None)), ("alignment", dict(dy=FAKE + 4)), ("alignment", dict(dx=FAKE + 4)),
                    ("alignment", dict(dres=FAKE + 8)), ("alignment", dict(dgamma=FAKE + 4)), ("alignment", dict(dbeta=FAKE + 4)),
                    ("alignment", dict(dbias=FAKE + 4)), ("stride", dict(ld_dy=766)), ("stride", dict(ld_dx=704)), ("stride", dict(ld_dres=2))):
        refused(bwd, lambda: L.ance_layer_tail_backward(ctypes.byref(tail_args()), ctypes.byref(tail_grads(**kw)), None), why)
    # the front end is shared with the 16-bit family: a missing dy keeps THIS family's text (not "neither dy nor dy16"), an fp32
    # stride its own rule's, and the arguments are judged before the gradients
    refused(bwd, lambda: L.ance_layer_tail_backward(ctypes.byref(tail_args()), ctypes.byref(tail_grads(dy=None)), None), "(null pointer)")
    refused(bwd, lambda: L.ance_layer_tail_backward(ctypes.byref(tail_args(eps=0.0)), ctypes.byref(tail_grads(dy=None)), None), "(eps <= 0)")
    refused(fwd, lambda: L.ance_layer_tail_forward(ctypes.byref(tail_args(ld_x=770)), None), "(stride: not a multiple of 4 or below the width)")

    fwd, bwd = "ance_bias_gelu_forward", "ance_bias_gelu_backward"
    for why, kw in GELU_REFUSALS + GELU_FORWARD_ONLY:
        refused(fwd, lambda: L.ance_bias_gelu_forward(ctypes.byref(gelu_args(**kw)), None), why)
    for why, kw in GELU_REFUSALS + GELU_BACKWARD_ONLY:
        refused(bwd, lambda: L.ance_bias_gelu_backward(ctypes.byref(gelu_args(**kw)), ctypes.byref(gelu_grads()), None), why)
    full = L.ance_bias_gelu_workspace_bytes(100, 3072)
    refused(bwd, lambda: L.ance_bias_gelu_backward(ctypes.byref(gelu_args(workspace_bytes=full - 1)), ctypes.byref(gelu_grads()), None), "workspace")
    assert L.ance_bias_gelu_forward(None, None) == -1
    refused(bwd, lambda: L.ance_bias_gelu_backward(ctypes.byref(gelu_args()), None, None), "null pointer")
    for why, kw in (("null pointer", dict(dy=None)), ("alignment", dict(dy=FAKE + 4)), ("alignment", dict(dx=FAKE + 8)),
                    ("alignment", dict(dbias=FAKE + 4)), ("stride", dict(ld_dy=3071)), ("stride", dict(ld_dx=1024))):
        refused(bwd, lambda: L.ance_bias_gelu_backward(ctypes.byref(gelu_args()), ctypes.byref(gelu_grads(**kw)), None), why)
