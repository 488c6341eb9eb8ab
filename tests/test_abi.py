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


def test_library_loads_exports_everything_at_abi_6():
    """ABI 6: + ance_debug_gemm_hw (include/ance_amd.h)."""
    L = _lib.lib()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in _declared_functions():
        assert hasattr(raw, name), name
    assert L.ance_abi_version() == _lib.ABI_VERSION == 6
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


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.AnceLibraryError):
        _lib.lib()
