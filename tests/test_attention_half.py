"""The 16-bit attention core without a GPU: the argument and dtype checks of precision="half" (ance_amd/attention.py), the refusals of
the C ABI (include/ance_amd.h: ance_attention16_*), the binding's struct layout, and the attainability of the GPU tests' bound: a
numpy model of the kernels' arithmetic contract stays within bound16 on every seeded case tests/test_gpu_attention_half.py runs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import attention_half_util as HU
import attention_train_util as A
from ance_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Cuda(torch.Tensor):
    """A CPU tensor that only claims is_cuda: reaches the host-side checks and nothing behind them."""
    is_cuda = True


def fake(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(Cuda)


# ---------------------------------------------------------------------------------------------------------------- Python checks
def test_precision_keyword_and_dtype_checks():
    from ance_amd import attention as T
    h, b, x = fake(2, 8, 768, dtype=torch.float16), fake(2, 8, 768, dtype=torch.bfloat16), fake(2, 8, 768)
    for bad in ("fp16", "bf16", None, 16):
        with pytest.raises(_lib.AnceLibraryError, match="precision"):
            T.attention_padded(h, h, h, None, 12, precision=bad)
        with pytest.raises(_lib.AnceLibraryError, match="precision"):
            T.attention_packed(h[0], h[0], h[0], None, 8, 12, precision=bad)
    # the default still refuses a half tensor by the name of float32
    with pytest.raises(_lib.AnceLibraryError, match="float32"):
        T.attention_padded(h, h, h, None, 12)
    with pytest.raises(_lib.AnceLibraryError, match="float32"):
        T._check_inputs(x, x, h, 12, 0.0, 3)
    # precision="half" outside autocast: fp32 (and anything else) is refused by the names of the two 16-bit types
    for t in (x, fake(2, 8, 768, dtype=torch.float64)):
        with pytest.raises(_lib.AnceLibraryError, match="float16 or bfloat16"):
            T.attention_padded(t, t, t, None, 12, precision="half")
    with pytest.raises(_lib.AnceLibraryError, match="float16 or bfloat16"):
        T._check_inputs(h, h, x, 12, 0.0, 3, half=True)
    T._check_inputs(h, h, h, 12, 0.0, 3, half=True)
    T._check_inputs(b, b, b, 12, 0.0, 3, half=True)
    with pytest.raises(_lib.AnceLibraryError, match="all be torch.float16 or all bfloat16"):
        T._half_inputs(h, b, h)
    assert all(t.dtype == torch.float16 for t in T._half_inputs(h, h, h))
    # the other checks are shared with the fp32 path
    for bad, why in ((dict(n_heads=8), "n_heads"), (dict(n_heads=16), "64 \\* n_heads"), (dict(dropout_p=1.0), "dropout_p")):
        kw = dict(dict(n_heads=12, dropout_p=0.0), **bad)
        with pytest.raises(_lib.AnceLibraryError, match=why):
            T._check_inputs(h, h, h, kw["n_heads"], kw["dropout_p"], 3, half=True)
    with pytest.raises(_lib.AnceLibraryError, match="1 .. 512"):
        T.attention_padded(fake(1, 513, 768, dtype=torch.float16), fake(1, 513, 768, dtype=torch.float16),
                           fake(1, 513, 768, dtype=torch.float16), None, 12, precision="half")


def test_rows16_accepts_strides_that_are_multiples_of_8():
    from ance_amd import attention as T
    fused = torch.zeros(2, 8, 3 * 768, dtype=torch.float16)
    for t in (fused[..., :768], fused[..., 768:1536], fused[..., 1536:]):
        kept, ld = T._rows(t, 8)
        assert ld == 3 * 768 and kept.data_ptr() == t.data_ptr()          # a view passes as it is
    odd = torch.zeros(2, 8, 768 + 4, dtype=torch.float16)[..., :768]     # stride 772: a multiple of 4, not of 8
    kept, ld = T._rows(odd, 8)
    assert ld == 768 and kept.is_contiguous()
    kept, ld = T._rows(torch.zeros(16, 776, dtype=torch.bfloat16)[:, :768], 8)
    assert ld == 776


def test_bert_layer_takes_attention_precision():
    from ance_amd.layers import BertLayer
    assert BertLayer(768, 12, 3072).attention_precision == "fp32"
    assert BertLayer(768, 12, 3072, attention_precision="half").attention_precision == "half"
    with pytest.raises(_lib.AnceLibraryError, match="attention_precision"):
        BertLayer(768, 12, 3072, attention_precision="fp16")


# ---------------------------------------------------------------------------------------------------------------- the binding
def test_struct_layout_matches_the_header(tmp_path):
    """sizeof and every offsetof of the two structs, from a C program compiled against include/ance_amd.h."""
    fields = {"AnceAttn16Args": [f for f, _ in _lib.AnceAttn16Args._fields_], "AnceAttn16GradArgs": [f for f, _ in _lib.AnceAttn16GradArgs._fields_]}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "ance_amd.h"', "int main(void) {"]
    for s, fs in fields.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f) for f in fs]
    lines += ['printf("ANCE_DTYPE_F16 %d\\nANCE_DTYPE_BF16 %d\\n", ANCE_DTYPE_F16, ANCE_DTYPE_BF16);', "return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if subprocess.run(
        ["sh", "-c", "command -v %s" % c], capture_output=True).returncode == 0), None)
    assert cc is not None, "no C compiler"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for s, cls in (("AnceAttn16Args", _lib.AnceAttn16Args), ("AnceAttn16GradArgs", _lib.AnceAttn16GradArgs)):
        assert int(got[s]) == ctypes.sizeof(cls), s
        for f in fields[s]:
            assert int(got["%s.%s" % (s, f)]) == getattr(cls, f).offset, (s, f)
    assert int(got["ANCE_DTYPE_F16"]) == _lib.ANCE_DTYPE_F16 == 1 and int(got["ANCE_DTYPE_BF16"]) == _lib.ANCE_DTYPE_BF16 == 2
    # the layout of the fp32 call's struct with dtype in the place of reserved
    assert [f for f, _ in _lib.AnceAttn16Args._fields_] == [("dtype" if f == "reserved" else f) for f, _ in _lib.AnceAttnTrainArgs._fields_]


# ---------------------------------------------------------------------------------------------------------------- C ABI refusals
def _args(**kw):
    fake_p = 0x10000
    a = _lib.AnceAttn16Args(q=fake_p, k=fake_p, v=fake_p, ctx=fake_p, ld_q=768, ld_k=768, ld_v=768, ld_ctx=768, d_seq_first=fake_p,
                            d_seq_len=fake_p, n_seq=2, max_seq_len=128, n_rows=256, n_heads=12, dtype=_lib.ANCE_DTYPE_F16, dropout_p=0.1,
                            training=1, seed=1, offset=0, d_workspace=fake_p, workspace_bytes=1 << 20)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _grads(**kw):
    fake_p = 0x10000
    g = _lib.AnceAttn16GradArgs(dctx=fake_p, dq=fake_p, dk=fake_p, dv=fake_p, ld_dctx=768, ld_dq=768, ld_dk=768, ld_dv=768)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def test_workspace_query_is_the_fp32_one():
    L = _lib.lib()
    for rows, nh in ((1000, 12), (1, 16), (8 * 512, 12), (1000, 8), (0, 12), (1 << 31, 12), (1000, 13)):
        assert L.ance_attention16_workspace_bytes(rows, nh) == L.ance_attention_workspace_bytes(rows, nh), (rows, nh)
    assert L.ance_attention16_workspace_bytes(8 * 512, 12) <= 2 * 4 * 8 * 512 * 12 + 512   # linear in the rows


def test_c_abi_refuses_before_any_launch():
    """Every refusal happens on the host: the pointers are fake and never dereferenced."""
    L = _lib.lib()

    def refused(why, fwd_too=True, grads=None, **kw):
        a = _args(**kw)
        g = grads if grads is not None else _grads()
        calls = [("ance_attention16_backward", lambda: L.ance_attention16_backward(ctypes.byref(a), ctypes.byref(g), None))]
        if fwd_too:
            calls.append(("ance_attention16_forward", lambda: L.ance_attention16_forward(ctypes.byref(a), None)))
        for fn, call in calls:
            rc, msg = call(), L.ance_last_error().decode()
            assert rc == -1 and fn in msg and why in msg, (fn, why, kw, rc, msg)

    assert L.ance_attention16_forward(None, None) == -1
    assert L.ance_attention16_backward(None, ctypes.byref(_grads()), None) == -1
    assert L.ance_attention16_backward(ctypes.byref(_args()), None, None) == -1 and b"null pointer" in L.ance_last_error()
    for d in (0, 3, -1, 16):
        refused("dtype", dtype=d)
    for f in ("q", "k", "v", "ctx", "d_seq_first", "d_seq_len"):
        refused("null pointer", **{f: None})
    for nh in (0, 8, 11, 13, 24):
        refused("n_heads", n_heads=nh)
    for m in (0, -1, 513, 1024):
        refused("max_seq_len", max_seq_len=m)
    for n in (0, -3, 65536):
        refused("n_seq", n_seq=n)
    refused("n_rows", n_rows=0)
    for r in (-1, 129, 512):
        refused("seq_rows", seq_rows=r)
    for f in ("ld_q", "ld_k", "ld_v", "ld_ctx"):
        for ld in (772, 764, 770, 767, 0, -768):   # 772 and 764 are multiples of 4: the fp32 call's rule is not enough
            refused("stride", **{f: ld})
    refused("stride", n_heads=16)  # the strides of 12 heads
    for f in ("q", "k", "v", "ctx"):
        for off in (4, 8, 2):
            refused("alignment", **{f: 0x10000 + off})
    for p in (-0.1, 1.0, 1.5, float("nan")):
        refused("dropout_p", dropout_p=p)
    refused("workspace", d_workspace=None)
    refused("workspace", d_workspace=0x10000 + 8)
    refused("workspace", workspace_bytes=L.ance_attention16_workspace_bytes(256, 12) - 1)
    for f in ("dctx", "dq", "dk", "dv"):
        refused("null pointer", fwd_too=False, grads=_grads(**{f: None}))
        refused("alignment", fwd_too=False, grads=_grads(**{f: 0x10000 + 4}))
        refused("stride", fwd_too=False, grads=_grads(**{"ld_" + f: 772}))
        refused("stride", fwd_too=False, grads=_grads(**{"ld_" + f: 704}))


# ---------------------------------------------------------------------------------------------------------------- the bound
def test_ulp16_and_bound16():
    assert HU.ulp16(1.0, torch.float16) == 2.0 ** -10 and HU.ulp16(1.999, torch.float16) == 2.0 ** -10
    assert HU.ulp16(2.0, torch.float16) == 2.0 ** -9 and HU.ulp16(1e-9, torch.float16) == 2.0 ** -24
    assert HU.ulp16(1.0, torch.bfloat16) == 2.0 ** -7 and HU.ulp16(300.0, torch.bfloat16) == 2.0
    for dt in (torch.float16, torch.bfloat16):   # against torch's own next representable value
        for x in (0.37, 1.0, 5.5, 1000.0):
            t = torch.tensor(x).to(dt)
            step = (t.view(torch.int16) + 1).view(dt).float() - t.float()
            assert float(step) == HU.ulp16(float(t), dt), (dt, x)
    assert HU.bound16(1.0, 1.0, torch.float16) == 4.0 and HU.bound16(0.0, 1.0, torch.float16) == 2.0 ** -9


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("case", range(len(HU.SEEDED_CASES)))
def test_the_contract_model_meets_the_bound_on_the_seeded_cases(case, dt):
    """kernel_model_half against fp64 within bound16 (lse: A.bound) on the seeded cases of the GPU file: the bound is attainable by
    the contract, so a GPU failure is the kernels' fault."""
    tag, lens, nh, L, q_scale, p = HU.SEEDED_CASES[case]
    (q, k, v, g, ln), want, ref, keep = HU.seeded_reference(tag, lens, nh, L, q_scale, p, HU.DROPOUT_SEED, 0, dt)
    got = HU.kernel_model_half(q, k, v, g, ln, nh, HU.DTYPES[dt], keep, p)
    HU.check("model %s %s p=%g" % (tag, dt, p), got, want, ref, HU.DTYPES[dt])


@pytest.mark.parametrize("lens,nh,dt", [(A.SWEEP_LENS, 12, "fp16"), (A.SWEEP_LENS_16, 16, "bf16")])
def test_the_contract_model_meets_the_bound_on_the_length_sweeps(lens, nh, dt):
    (q, k, v, g, ln), want, ref = HU.sweep_reference(lens, nh, dt)
    got = {n: np.zeros_like(want[n], dtype=np.float32) for n in A.NAMES}
    L = q.shape[1]
    for b, n in enumerate(lens):
        r = HU.kernel_model_half(*[x[b:b + 1, :n] for x in (q, k, v, g)], [n], nh, HU.DTYPES[dt])
        for name in ("ctx", "dq", "dk", "dv"):
            got[name][b, :n] = r[name][0]
        got["lse"][:, b * L:b * L + n] = r["lse"]
    HU.check("model sweep %d heads %s" % (nh, dt), got, want, ref, HU.DTYPES[dt])


def test_the_contract_model_is_exact_on_the_one_hot_case():
    for n in (32, 96):
        q, k, v, g, pi = HU.one_hot_case(n)
        got = HU.kernel_model_half(q, k, v, g, [n], 12, torch.float16)
        for h in range(12):
            c = slice(64 * h, 64 * h + 64)
            assert np.array_equal(got["ctx"][0, :, c], v[0, pi[h], c]) and np.all(got["lse"][h] == 504.0)
            assert np.array_equal(got["dv"][0, pi[h], c], g[0, :, c])
        assert np.all(got["dq"] == 0) and np.all(got["dk"] == 0)
