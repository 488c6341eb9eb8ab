"""Encoder throughput of the large tower (RoBERTa-large width: 24 layers, hidden 1024, 16 heads, FFN 4096) beside the base tower
(12 layers, 768 / 12 / 3072), in the same process, in the three arithmetic modes.  Prints ONE JSON line.

    python scripts/bench_large.py [--block 16384] [--steps 3] [--warmup 1]

Workload per step: one ance_encode_records call on --block resident passages, L = 128, lengths of bench.py's encode leg
(lognormal, median 70, sigma 0.45, clipped to [8, 128]), 131,072-token micro-batches, random-init weights (std 0.02).
Per tower and mode: passages/s, algorithmic TF/s (per sequence of T tokens
n_layers (8 H^2 + 4 H I) T + 4 n_layers H T^2 + 2 H 768 FLOP; large: 603,979,776 T + 98,304 T^2 + 1,572,864) and the per-category
kernel times of one extra step with the library's profile hook on (ance_profile_read; the timed steps run without it).
``tfs_ratio_large_vs_base`` is the large tower's algorithmic TF/s over the base tower's, per mode."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOWERS = {"large": dict(n_layers=24, hidden=1024, inter=4096), "base": dict(n_layers=12, hidden=768, inter=3072)}


def flops_per_sequence(T, n_layers, hidden, inter):
    T = np.asarray(T, dtype=np.float64)
    return n_layers * (8.0 * hidden * hidden + 4.0 * hidden * inter) * T + 4.0 * n_layers * hidden * T * T + 2.0 * hidden * 768


def records(rng, n, L):
    """Tokenised-cache rows [n, 1 + L] int32 (big-endian length header, <s> ... </s>, pad 1) -- bench.py's encode-leg draw."""
    lens = np.clip(np.rint(rng.lognormal(np.log(70.0), 0.45, size=n)), 8, L).astype(np.int32)
    ids = rng.integers(3, 50265, size=(n, L), dtype=np.int64).astype(np.int32)
    ids[:, 0] = 0
    ids[np.arange(n), lens - 1] = 2
    ids = np.where(np.arange(L)[None, :] < lens[:, None], ids, 1).astype(np.int32)
    rec = np.empty((n, 1 + L), dtype=np.int32)
    rec[:, 0] = lens.astype(">u4").view(np.int32)
    rec[:, 1:] = ids
    return rec, lens


def random_state_dict(torch, n_layers, hidden, inter, dev, seed=0):
    """Random-init rdot_nll weights on the device (normal std 0.02, LayerNorm 1 / 0, biases 0: model/models.py:31-36)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    sd = {}

    def rnd(*shape):
        return torch.randn(*shape, generator=g, device=dev) * 0.02

    def lin(name, o, i):
        sd[name + ".weight"], sd[name + ".bias"] = rnd(o, i), torch.zeros(o, device=dev)

    def ln(name, n=hidden):
        sd[name + ".weight"], sd[name + ".bias"] = torch.ones(n, device=dev), torch.zeros(n, device=dev)

    e = "roberta.embeddings."
    sd[e + "word_embeddings.weight"] = rnd(50265, hidden)
    sd[e + "position_embeddings.weight"] = rnd(514, hidden)
    sd[e + "token_type_embeddings.weight"] = rnd(1, hidden)
    ln(e + "LayerNorm")
    for i in range(n_layers):
        p = "roberta.encoder.layer.%d." % i
        for k in ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense"):
            lin(p + k, hidden, hidden)
        ln(p + "attention.output.LayerNorm")
        lin(p + "intermediate.dense", inter, hidden)
        lin(p + "output.dense", hidden, inter)
        ln(p + "output.LayerNorm")
    lin("embeddingHead", 768, hidden)
    ln("norm", 768)
    return sd


def measure(torch, enc, rec, lens, steps, warmup):
    from ance_amd import _lib
    out = torch.empty((rec.shape[0], 768), dtype=torch.float32, device="cuda")
    rec_d = torch.from_numpy(rec).cuda()
    for _ in range(warmup):
        enc.encode_records(rec_d, h_lens=lens, out=out)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        enc.encode_records(rec_d, h_lens=lens, out=out)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    enc.check_range(sync=True)
    # one profiled step: per-category kernel time (ms) and launch count
    before = _lib.profile_read()
    _lib.profile_enable(True)
    enc.encode_records(rec_d, h_lens=lens, out=out)
    torch.cuda.synchronize()
    after = _lib.profile_read()
    _lib.profile_enable(False)
    cats = {c: dict(ms=round(after[c]["ms"] - before[c]["ms"], 4), count=after[c]["count"] - before[c]["count"])
            for c in after if after[c]["count"] > before[c]["count"]}
    return dt, cats, bool(torch.isfinite(out).all())


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--block", type=int, default=16384, help="passages per encode call")
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--seq-len", type=int, default=128)
    p.add_argument("--max-tokens", type=int, default=131072)
    a = p.parse_args()
    import torch
    from ance_amd.encoder import ARCH_ROBERTA, Encoder
    rng = np.random.default_rng(0)
    rec, lens = records(rng, a.block, a.seq_len)
    res = {}
    for tower, shape in TOWERS.items():
        sd = random_state_dict(torch, shape["n_layers"], shape["hidden"], shape["inter"], "cuda")
        flop = float(flops_per_sequence(lens, **shape).sum())
        res[tower] = dict(shape)
        for mode in ("split", "fp16", "fp32"):
            enc = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=a.seq_len, max_tokens=a.max_tokens, precision=mode)
            dt, cats, finite = measure(torch, enc, rec, lens, a.steps, a.warmup)
            res[tower][mode] = dict(passages_per_s=round(a.block / dt, 1), tflops_algorithmic=round(flop / dt / 1e12, 2),
                                    ms_per_step=round(dt * 1e3, 3), finite=finite, kernel_ms=cats)
            del enc
            torch.cuda.empty_cache()
        del sd
        torch.cuda.empty_cache()
    ratio = {m: round(res["large"][m]["tflops_algorithmic"] / res["base"][m]["tflops_algorithmic"], 4) for m in ("split", "fp16", "fp32")}
    print(json.dumps(dict(bench="bench_large", device=torch.cuda.get_device_name(0), block=a.block, seq_len=a.seq_len,
                          max_tokens=a.max_tokens, steps=a.steps, warmup=a.warmup,
                          mean_tokens_per_passage=float(lens.mean()), towers=res, tfs_ratio_large_vs_base=ratio)))


if __name__ == "__main__":
    main()
