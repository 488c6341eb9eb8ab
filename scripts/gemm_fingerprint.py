#!/usr/bin/env python
"""SHA-256 fingerprints of the raw output buffers of the 256 x 256 GEMM's three test hooks on fixed-seed inputs: the check that a
restructuring of the GEMM source moved no bit, at kernel level -- scripts/encoder_fingerprint.py runs a random-init model, which
never takes the folded GEMMs' second pass over a wide-mean token's lo halves, and reaches the hooks' marshalling not at all.

    python scripts/gemm_fingerprint.py                          # {"case": sha256, ...} of the library in the tree (or ANCE_AMD_LIB)
    python scripts/gemm_fingerprint.py --libs A.so B.so --out F  # one fresh child process per library; exit 1 unless all agree

Cases (each at the smallest shape that reaches the code):
  ance_debug_gemm        epi 0, 1, 2 at (256, 256, 128)
  ance_debug_gemm_split  epi 8, 9 at (256, 256, 128); epi 10 at N = 768 and 1024 (with part_out); epi 8 and 9 at (8448, 2048, 128)
                         with ANCE_GEMM_STREAM = 1 and 0: 33 M-tiles padded to 40, times 8 N-tiles = 320 virtual blocks on 256 CUs,
                         so persistent workgroups take a second tile through the hand-over and skip padding blocks
  ance_debug_gemm_hw     at hidden 768 and 1024: epi 4 (RESLN, hi / lo / part_out); epi 5, 6, 7 with tok_lo and a token with
                         |mean| rstd > 2 in every tile, so that the masked second pass runs; epi 6 and 9 with n_split = 2 at
                         (256, 512, 128)
A NaN in any output fails the run.  The operands are built by the helpers of tests/test_gpu_gemm.py and tests/test_gpu_gemm_fold.py."""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def fingerprints():
    import torch
    from ance_amd import _lib
    import test_gpu_gemm as tg
    import test_gpu_gemm_fold as tf

    L = _lib.lib()
    out = {}
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def record(name, **bufs):
        torch.cuda.synchronize()
        for k, t in bufs.items():
            assert not bool(torch.isnan(t.float()).any()), "%s/%s: NaN in the output" % (name, k)
            raw = t.contiguous().view(torch.uint8).cpu().numpy().tobytes()
            out["%s/%s" % (name, k)] = hashlib.sha256(raw).hexdigest()

    def stream(mode):
        os.environ["ANCE_GEMM_STREAM"] = mode
        _lib.reload_env()

    def gen(seed):
        return torch.Generator(device="cuda").manual_seed(seed)

    # ---- ance_debug_gemm: the plain epilogues ----
    for epi in (0, 1, 2):
        M, N, K = 256, 256, 128
        g = gen(100 + epi)
        a = (torch.randn((M, K), generator=g, device="cuda") * 0.5).half()
        b = (torch.randn((N, K), generator=g, device="cuda") * 0.5).half()
        bias = torch.randn(N, generator=g, device="cuda")
        res = torch.randn((M, N), generator=g, device="cuda") if epi == 2 else None
        o = torch.zeros((M, N), dtype=torch.float32 if epi == 2 else torch.float16, device="cuda")
        _lib.check(L.ance_debug_gemm(0, epi, P(a), P(b), M, N, K, P(bias), P(o), P(res), _lib.current_stream_ptr()), "ance_debug_gemm")
        record("gemm/epi%d" % epi, out=o)

    # ---- ance_debug_gemm_split ----
    def split(name, epi, M, N, K, seed, wscale=2.0 ** 13):
        g = gen(seed)
        ap = tg._pair_rows(*tg._pair(torch.randn((M, K), generator=g, device="cuda")))
        bp = tg._pair_rows(*tg._pair(torch.randn((N, K), generator=g, device="cuda") * 0.02 * wscale))
        winv = torch.tensor([1.0 / wscale], dtype=torch.float32, device="cuda")
        bias, vec1, vec2 = (torch.randn(N, generator=g, device="cuda") for _ in range(3))
        hw = 1024 if (epi == 10 and N == 1024) else 768
        ns, cols = tg.part_format(hw)
        part = torch.zeros((M, 24), device="cuda")
        part[:, 0:2 * ns:2] = torch.randn((M, ns), generator=g, device="cuda") * 0.1
        part[:, 1:2 * ns:2] = cols * (0.5 + torch.rand((M, ns), generator=g, device="cuda"))
        rp = tg._pair_rows(*tg._pair(torch.randn((M, N), generator=g, device="cuda")))
        o = torch.zeros((M, N), dtype=torch.float32, device="cuda") if epi == 8 else torch.zeros((M, 2 * N), dtype=torch.float16, device="cuda")
        part_out = torch.zeros((M, 24), device="cuda")
        _lib.check(L.ance_debug_gemm_split(epi, P(ap), P(bp), M, N, K, P(bias), P(vec1), P(vec2), P(part), 1e-5, P(rp), P(o), P(part_out),
                                           P(winv), _lib.current_stream_ptr()), "ance_debug_gemm_split")
        if epi == 10:
            record(name, out=o, part_out=part_out)
        else:
            record(name, out=o)

    try:
        for epi in (8, 9):
            split("split/epi%d" % epi, epi, 256, 256, 128, 200 + epi)
        for N in (768, 1024):
            split("split/epi10_N%d" % N, 10, 256, N, 128, 210 + N)
        for mode in ("1", "0"):
            stream(mode)
            for epi in (8, 9):
                split("split/epi%d_8448x2048_stream%s" % (epi, mode), epi, 8448, 2048, 128, 220 + epi)
    finally:
        os.environ.pop("ANCE_GEMM_STREAM", None)
        _lib.reload_env()

    # ---- ance_debug_gemm_hw: the encoder's instances at both hidden widths ----
    def wide_in_every_tile(n):
        r = torch.zeros(n, dtype=torch.float64)
        for t in range(n // 256):
            r[t * 256 + 5 + 17 * t] = 30.0 if t % 2 == 0 else 2.1
            r[t * 256 + 140] = 1.9
        return r

    for hw in (768, 1024):
        # RESLN
        M, N, K = 256, hw, 128
        g = gen(300 + hw)
        a = (torch.randn((M, K), generator=g, device="cuda") * 0.5).half()
        w, _, bias = tf._weights(N, K, 301 + hw)
        rhi, rlo, part, _ = tf.token_rows(M, hw, 302 + hw, ratios=wide_in_every_tile(M))
        gamma = 1.0 + 0.2 * torch.randn(N, generator=g, device="cuda")
        beta = 0.1 * torch.randn(N, generator=g, device="cuda")
        hi = torch.zeros((M, N), dtype=torch.float16, device="cuda")
        lo = torch.zeros_like(hi)
        part_out = torch.zeros((M, 24), device="cuda")
        tf.gemm_hw(4, hw, a=a, b=w, lda=K, ldb=K, M=M, N=N, K=K, bias=bias, part_in=part, res_hi=rhi, res_lo=rlo, res_gamma=gamma,
                   res_beta=beta, out=hi, out_lo=lo, part_out=part_out, ldc=N)
        record("hw%d/epi4" % hw, out=hi, out_lo=lo, part_out=part_out)

        # folded A-side epilogues with the masked second pass: two token tiles, two feature tiles (one inside scale_cols)
        for epi in (5, 6):
            M, N = 512, 512
            thi, tlo, part, wide = tf.token_rows(M, hw, 310 + hw + epi, ratios=wide_in_every_tile(M))
            assert bool(wide[:256].any()) and bool(wide[256:].any())
            w, csum, bias = tf._weights(N, hw, 311 + hw + epi)
            o = torch.zeros((M, N), dtype=torch.float16, device="cuda")
            tf.gemm_hw(epi, hw, a=thi, b=w, lda=hw, ldb=hw, M=M, N=N, K=hw, bias=bias, csum=csum, part_in=part, tok_lo=tlo,
                       scale=0.125 if epi == 5 else 1.0, scale_cols=256 if epi == 5 else 0, out=o, ldc=N)
            record("hw%d/epi%d_tok_lo" % (hw, epi), out=o)

        # folded V^T: tokens are the B rows, scattered through a col_map
        n_tok, n_valid = 512, 450
        thi, tlo, part, wide = tf.token_rows(n_tok, hw, 320 + hw, ratios=wide_in_every_tile(n_tok))
        w, csum, bias = tf._weights(hw, hw, 321 + hw)
        col_map, ldc = tf._vt_layout(n_tok, n_valid, 322 + hw)
        o = torch.zeros((hw, ldc), dtype=torch.float16, device="cuda")
        tf.gemm_hw(7, hw, a=w, b=thi, lda=hw, ldb=hw, M=hw, N=n_tok, K=hw, bias=bias, csum=csum, part_in=part, tok_lo=tlo,
                   col_map=col_map, n_valid=n_valid, out=o, ldc=ldc)
        record("hw%d/epi7_tok_lo" % hw, out=o)

        # N-split tile order
        M, N, K = 256, 512, 128
        ns, cols = tg.part_format(hw)
        g = gen(330 + hw)
        part = torch.zeros((M, 24), device="cuda")
        part[:, 0:2 * ns:2] = torch.randn((M, ns), generator=g, device="cuda") * 0.1
        part[:, 1:2 * ns:2] = cols * (0.5 + torch.rand((M, ns), generator=g, device="cuda"))
        a = (torch.randn((M, K), generator=g, device="cuda") * 0.5).half()
        w, csum, bias = tf._weights(N, K, 331 + hw)
        o = torch.zeros((M, N), dtype=torch.float16, device="cuda")
        tf.gemm_hw(6, hw, a=a, b=w, lda=K, ldb=K, M=M, N=N, K=K, bias=bias, csum=csum, part_in=part, out=o, ldc=N, n_split=2)
        record("hw%d/epi6_n_split" % hw, out=o)
        ap = tg._pair_rows(*tg._pair(torch.randn((M, K), generator=g, device="cuda")))
        w, csum, bias = tf._weights(N, K, 332 + hw, scale=0.02 * 2.0 ** 13)
        bp = tg._pair_rows(*tg._pair(w.float()))
        winv = torch.tensor([2.0 ** -13], device="cuda")
        o = torch.zeros((M, 2 * N), dtype=torch.float16, device="cuda")
        tf.gemm_hw(9, hw, a=ap, b=bp, lda=2 * K, ldb=2 * K, M=M, N=N, K=K, bias=bias, csum=csum * 2.0 ** -13, part_in=part, out=o,
                   ldc=2 * N, wscale_inv=winv, n_split=2)
        record("hw%d/epi9_n_split" % hw, out=o)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs="+", help="libraries to compare (ANCE_AMD_LIB of one fresh child process each)")
    ap.add_argument("--out", help="write the result as JSON")
    a = ap.parse_args()
    if not a.libs:
        res = fingerprints()
    else:
        res = {}
        for lib in a.libs:
            env = dict(os.environ, ANCE_AMD_LIB=os.path.abspath(lib))
            p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.PIPE, text=True, timeout=600)
            if p.returncode != 0:
                sys.exit("fingerprint run of %s failed (%d)" % (lib, p.returncode))
            res[lib] = json.loads(p.stdout.strip().splitlines()[-1])
        first = res[a.libs[0]]
        res["unequal"] = sorted(k for lib in a.libs[1:] for k in set(first) | set(res[lib]) if first.get(k) != res[lib].get(k))
    text = json.dumps(res, indent=1, sort_keys=True) if a.out else json.dumps(res, sort_keys=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    if a.libs and res["unequal"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
