"""The C-ABI shared library loads on a CPU-only box and exports every symbol include/ance_amd.h
declares; argument validation (which never touches a device) behaves as documented."""
import ctypes
import os
import re

import pytest

from ance_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions():
    src = open(os.path.join(ROOT, "include", "ance_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b(ance_[a-z0-9_]+)\s*\(", src)
    return sorted(set(names))


def test_header_and_binding_agree():
    declared = _declared_functions()
    assert declared, "no functions parsed from the header"
    assert sorted(_lib.SYMBOLS.keys()) == declared


def test_library_loads_exports_everything_at_abi_7():
    """ABI 7: + ance_debug_attention (include/ance_amd.h)."""
    L = _lib.lib()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in _declared_functions():
        assert hasattr(raw, name), name
    assert L.ance_abi_version() == _lib.ABI_VERSION == 7
    assert L.ance_last_error() is not None


def test_workspace_queries_are_pure():
    L = _lib.lib()
    assert L.ance_ip_topk_workspace_bytes(10000, 1000, 768, 200) > 0
    assert L.ance_ip_topk_workspace_bytes(10000, 1000, 768, 0) == 0          # k out of range
    assert L.ance_ip_topk_workspace_bytes(10000, 1000, 768, 5000) == 0
    assert L.ance_ip_topk_workspace_bytes(1 << 33, 10, 768, 10) == 0         # n >= 2^32
    d = _lib.AnceEncoderDesc(arch=0, n_layers=12, hidden=768, n_heads=12, intermediate=3072, vocab_size=50265,
                             max_position=514, pad_token_id=1, ln_eps=1e-5, has_head=1, max_seq_len=512, max_tokens=32768)
    assert L.ance_encoder_weight_bytes(ctypes.byref(d)) > 300e6
    assert L.ance_encoder_workspace_bytes(ctypes.byref(d)) > 100e6
    d.hidden = 1024
    assert L.ance_encoder_weight_bytes(ctypes.byref(d)) == 0
    assert abs(L.ance_encoder_flops_per_sequence(128) - 22.35e9) / 22.35e9 < 1e-3
    assert abs(L.ance_encoder_flops_per_sequence(512) - 96.64e9) / 96.64e9 < 1e-3


def test_invalid_arguments_are_rejected_before_any_launch():
    L = _lib.lib()
    # null pointers / bad k: must return ANCE_E_INVALID without touching a device
    rc = L.ance_ip_topk(None, 10, 0, None, 4, 768, 0, None, None, None, 0, None)
    assert rc == -1 and b"invalid" in L.ance_last_error()
    rc = L.ance_topk_merge(None, None, 2, 4, 10, None, None, None, 0, None)
    assert rc == -1
    rc = L.ance_encode_records(None, None, None, 4, 128, 1, None, None)
    assert rc == -1
    rc = L.ance_nll_forward(None, None, None, None, None, 4, 768, 1, None, None, None, None)
    assert rc == -1 and b"nll" in L.ance_last_error()
    rc = L.ance_debug_gemm_split(8, None, None, 256, 256, 128, None, None, None, None, 1e-5, None, None, None, None, None)
    assert rc == -1
    rc = L.ance_ip_topk_scan(None, 10, 0, None, 4, 768, 0, None, None, None, 0, None)
    assert rc == -1 and b"invalid" in L.ance_last_error()
    assert L.ance_ip_topk_scan_workspace_bytes(10000, 1000, 768, 200) > 0
    assert L.ance_ip_topk_scan_workspace_bytes(10000, 1000, 768, 0) == 0
    assert L.ance_encoder_range_faults(None, None, 0, None) == -1
    _gemm_hw_refusals(L)
    assert L.ance_encoder_precision(None) == -1


def _gemm_hw_refusals(L):
    """ance_debug_gemm_hw: every refusal happens on the host, before a launch (the pointers below are never dereferenced)."""
    fake = ctypes.c_void_p(0x1000)

    def args(**kw):
        a = _lib.AnceGemmDebugArgs(a=fake, b=fake, lda=1024, ldb=1024, M=256, N=1024, K=1024, bias=fake, csum=fake, part_in=fake,
                                   ln_eps=1e-5, scale=1.0, col_map=fake, n_valid=256, ldc=1024, out=fake, res_hi=fake, res_lo=fake,
                                   res_gamma=fake, res_beta=fake, out_lo=fake, part_out=fake, ldr=2048)
        for k, v in kw.items():
            setattr(a, k, v)
        return ctypes.byref(a)

    def refused(epi, hw, a):
        rc = L.ance_debug_gemm_hw(epi, hw, a, None)
        return rc == -1 and b"ance_debug_gemm_hw" in L.ance_last_error()

    assert refused(5, 768, None)
    for hw in (0, 512, 767, 1023, 2048):
        assert refused(5, hw, args())
    for epi in (-1, 0, 1, 2, 3, 11, 12):
        assert refused(epi, 1024, args())
    for ns in (-1, 1, 3, 4):
        assert refused(6, 1024, args(n_split=ns))
    for epi in range(4, 11):
        for field in ("a", "b", "bias", "part_in", "out"):
            assert refused(epi, 1024, args(**{field: None})), (epi, field)
    for epi in (5, 6, 7, 8, 9):
        assert refused(epi, 768, args(csum=None)), epi
    assert refused(7, 1024, args(col_map=None))
    assert refused(5, 1024, args(scale_cols=100))
    for field in ("res_hi", "res_lo", "out_lo", "res_gamma", "res_beta", "part_out"):
        assert refused(4, 1024, args(**{field: None})), field
    for field in ("res_hi", "res_gamma", "res_beta", "part_out"):
        assert refused(10, 1024, args(**{field: None})), field
    assert refused(4, 768, args(N=1024)) and refused(10, 1024, args(N=768))  # the partials need N = hw
    # shapes the kernel cannot tile: refused by the launcher, still before any launch
    assert L.ance_debug_gemm_hw(5, 1024, args(M=300), None) == -1
    assert L.ance_debug_gemm_hw(5, 1024, args(K=64), None) == -1
    assert L.ance_debug_gemm_hw(6, 1024, args(N=768, n_split=2), None) == -1  # three N tiles: no N-split order


def test_attention_hook_refuses_before_any_launch():
    """ance_debug_attention: every refusal of include/ance_amd.h happens on the host, before the descriptor copy or a launch (the
    device pointers below are fake and never dereferenced; the descriptors are real host memory, which the hook reads)."""
    import numpy as np
    L = _lib.lib()
    fake = 0x10000

    def call(kind=0, nh=12, desc=((0, 100, 0, 0), (104, 64, 104, 1)), **kw):
        H = 64 * nh
        d = np.ascontiguousarray(np.array(desc, dtype=np.int32))
        n = len(desc) - 1 if kind == 2 else len(desc)
        a = _lib.AnceAttnDebugArgs(kind=kind, n_heads=nh, n_seq=n, max_seq_len=128, cls_only=0, q_compact=0,
                                   h_desc=d.ctypes.data, d_desc=fake, d_desc_bytes=4096, qk=fake,
                                   ld_qk=2 * H if kind == 0 else 3 * H, qk_rows=512, vt=fake, ld_vt=512, ctx=fake,
                                   ld_ctx=2 * H if kind == 1 else H, ctx_rows=512)
        for k, v in kw.items():
            setattr(a, k, v)
        return L.ance_debug_attention(ctypes.byref(a), None), L.ance_last_error().decode()

    def refused(why, **kw):
        rc, msg = call(**kw)
        assert rc == -1 and "ance_debug_attention" in msg and why in msg, (why, kw, rc, msg)

    assert L.ance_debug_attention(None, None) == -1
    for kind in (-1, 3, 7):
        refused("kind", kind=kind)
    for nh in (0, 8, 11, 13, 24):
        refused("n_heads", nh=nh)
    refused("n_seq", n_seq=0)
    for m in (0, -1, 513, 1024):
        refused("max_seq_len", max_seq_len=m)
    seqoff = (0, 100, 164)
    for kind, desc in ((0, None), (1, None), (2, seqoff)):
        kw = dict(kind=kind) if desc is None else dict(kind=kind, desc=desc)
        for field in ("h_desc", "d_desc", "qk", "ctx"):
            refused("null pointer", **dict(kw, **{field: None}))
        refused("d_desc", **dict(kw, d_desc_bytes=16 if kind != 2 else 8))
        refused("d_desc", **dict(kw, d_desc=fake + 4))
        refused("alignment", **dict(kw, qk=fake + 8))
        refused("alignment", **dict(kw, ctx=fake + 4))
    refused("null pointer", vt=None)
    refused("alignment", vt=fake + 2)
    # lengths outside 1 .. max_seq_len
    for ln in (0, -3, 129):
        refused("length", desc=((0, ln, 0, 0),))
        refused("length", kind=1, desc=((0, ln, 0, 0),))
    refused("length", kind=2, desc=(0, 0, 10))
    refused("length", kind=2, desc=(0, 129))
    refused("length", kind=2, desc=(5, 3))
    # tokens, Q row s, output rows and V^T columns past their allocations
    refused("tokens", desc=((450, 63, 0, 0),))
    refused("tokens", desc=((-1, 10, 0, 0),))
    refused("tokens", kind=1, desc=((0, 100, 0, 0), (500, 13, 0, 1)))
    refused("tokens", kind=2, desc=(400, 500, 513))
    refused("tokens", kind=2, desc=(-8, 10))
    refused("output row", desc=((0, 100, 0, 0),), ctx_rows=99)
    refused("output row", kind=1, desc=((0, 100, 0, 0),), ctx_rows=99)
    refused("tokens", kind=2, desc=(0, 100), ctx_rows=99)
    one_of_300 = tuple((i, 1, 8 * i, i) for i in range(300))
    refused("Q row s", desc=((0, 1, 0, 2), (1, 1, 8, 1), (0, 1, 16, 0)), cls_only=1, q_compact=1, qk_rows=2)
    refused("Q row s", kind=1, desc=((0, 1, 0, 2), (1, 1, 8, 1), (0, 1, 16, 0)), cls_only=1, q_compact=1, qk_rows=2)
    refused("output row", desc=one_of_300, cls_only=1, ctx_rows=299, ld_vt=4096, d_desc_bytes=16 * 300)
    refused("V^T columns", desc=((0, 100, 8, 0),), ld_vt=104)      # 8 + roundup8(100) = 112 > 104
    refused("V^T columns", desc=((0, 97, 16, 0),), ld_vt=112)     # 16 + roundup8(97) = 120: the gap columns count
    refused("V^T columns", desc=((0, 100, 4, 0),))                  # vcol % 8
    refused("V^T columns", desc=((0, 100, -8, 0),))
    # strides: 16-byte pieces (kind 0), fixed by n_heads (kinds 1, 2)
    for f, v in (("ld_qk", 1532), ("ld_qk", 1540), ("ld_vt", 516), ("ld_ctx", 764), ("ld_ctx", 772)):
        refused("stride", **{f: v})
    for kind in (1, 2):
        desc = None if kind == 1 else seqoff
        kw = dict(kind=kind) if desc is None else dict(kind=kind, desc=desc)
        refused("stride", **dict(kw, ld_qk=3 * 768 + 8))
        refused("stride", **dict(kw, ld_ctx=(None, 2 * 768, 768)[kind] + 8))
        refused("stride", **dict(kw, nh=16, ld_qk=3 * 768, ld_ctx=(None, 2 * 768, 768)[kind]))  # strides of 12 heads
    # sequence indices: repeated or out of range
    refused("sequence index", desc=((0, 100, 0, 0), (104, 64, 104, 0)))
    refused("sequence index", desc=((0, 100, 0, 0), (104, 64, 104, 2)))
    refused("sequence index", kind=1, desc=((0, 100, 0, -1), (104, 64, 104, 1)))
    # modes the kernels do not have
    refused("cls_only on kind 2", kind=2, desc=seqoff, cls_only=1)
    refused("cls_only on kind 2", kind=2, desc=seqoff, cls_only=1, q_compact=1)
    refused("kind 1: q_compact != cls_only", kind=1, cls_only=1)
    refused("kind 1: q_compact != cls_only", kind=1, q_compact=1)
    refused("q_compact without cls_only", q_compact=1)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.AnceLibraryError):
        _lib.lib()
