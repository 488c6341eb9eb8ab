"""Times the trainers' self-attention core (one layer's worth: from the three Linear outputs to context_layer, all heads) with device
events, in ONE process, the variants alternated --rounds times (each round times every variant once: --steps calls after --warmup):
  (a) eager   transformers 2.3.0's expression: matmul, / 8, additive mask, softmax, dropout, matmul -- the reference's only path
  (b) sdpa    torch.nn.functional.scaled_dot_product_attention with the same additive mask and dropout: a yardstick only
  (c) fused   ance_amd.attention.attention_padded -> csrc/attention_train.hip
Each variant runs the step's tower calls one after another, as the trainers do (query batch, positive batch, negative batch: each
its own padded [B, L, H] with its own lengths), in training mode with the reference's attention dropout (0.1), fp32.
Per variant and shape: forward alone, forward + backward, torch.cuda.max_memory_allocated over the pair above what was allocated
before it, and the launches of one forward + backward traced with torch.profiler (after the timing).  For (c) also the achieved share
of the 157.3 TFLOP/s fp32 matrix peak, counting the algorithm's 2 + 5 products over the VALID rows (the kernels execute 2 + 7: the
backward recomputes the scores in both of its passes).
Shapes, from the reference's launch recipes (triplet towers concatenated), with seeded length draws, not all-max:
  warmup   32 x (64, 128, 128)        commands/run_train_warmup.sh; MS MARCO passages, queries of 4..20 tokens
  firstp   8 x (64, 512, 512)         documents: 70 % fill the 512 window
  maxp     2 x (64 + 2 x 8 chunks of 512)   documents of 300..4096 tokens: full chunks, one partial chunk, all-pad chunks
  dpr      16 x (256, 256, 256)       questions of 6..30 tokens, passages of 100..256
Writes one JSON object (--out)."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_HEADS, H, P_DROP, PEAK_F32_MATRIX = 12, 768, 0.1, 157.3e12


def shapes(seed=0):
    """{name: [(L, lens), ...]}: the tower calls of one step."""
    import numpy as np
    rng = np.random.default_rng(seed)

    def passages(n, L, lo, mean, sd):
        return np.clip(rng.normal(mean, sd, n).round(), lo, L).astype(np.int32)

    def docs512(n):
        return np.where(rng.random(n) < 0.7, 512, rng.integers(100, 512, n)).astype(np.int32)

    def chunks(n_docs, n_chunks):
        out = []
        for t in rng.integers(300, 4097, n_docs):
            out += [int(min(max(t - 512 * c, 0), 512)) for c in range(n_chunks)]
        return np.asarray(out, np.int32)

    q = lambda n, lo, hi: rng.integers(lo, hi + 1, n).astype(np.int32)  # noqa: E731
    return {
        "warmup": [(64, q(32, 4, 20)), (128, passages(32, 128, 16, 75, 30)), (128, passages(32, 128, 16, 75, 30))],
        "firstp": [(64, q(8, 4, 20)), (512, docs512(8)), (512, docs512(8))],
        "maxp": [(64, q(2, 4, 20)), (512, chunks(2, 8)), (512, chunks(2, 8))],
        "dpr": [(256, q(16, 6, 30)), (256, passages(16, 256, 100, 180, 50)), (256, passages(16, 256, 100, 180, 50))],
    }


def eager(q, k, v, add_mask, lens, training):
    import torch
    B, L, _ = q.shape

    def tfs(x):
        return x.view(B, L, N_HEADS, 64).permute(0, 2, 1, 3)

    s = torch.matmul(tfs(q), tfs(k).transpose(-1, -2)) / math.sqrt(64) + add_mask
    p = torch.nn.functional.dropout(torch.softmax(s, dim=-1), P_DROP, training)
    return torch.matmul(p, tfs(v)).permute(0, 2, 1, 3).contiguous().view(B, L, H)


def sdpa(q, k, v, add_mask, lens, training):
    import torch
    B, L, _ = q.shape

    def tfs(x):
        return x.view(B, L, N_HEADS, 64).permute(0, 2, 1, 3)

    o = torch.nn.functional.scaled_dot_product_attention(tfs(q), tfs(k), tfs(v), attn_mask=add_mask, dropout_p=P_DROP if training else 0.0)
    return o.permute(0, 2, 1, 3).contiguous().view(B, L, H)


def fused(q, k, v, add_mask, lens, training):
    from ance_amd.attention import attention_padded
    return attention_padded(q, k, v, lens, N_HEADS, P_DROP, training)


VARIANTS = {"eager": eager, "sdpa": sdpa, "fused": fused}


def time_calls(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def traced_launches(fn):
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    kernels = copies = 0
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            if "memcpy" in e.name.lower() or "memset" in e.name.lower():
                copies += 1
            else:
                kernels += 1
    return dict(kernels=kernels, copies_and_memsets=copies)


def bench(name, calls, rounds, steps, warmup, trace):
    import torch
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    data = []
    for L, lens in calls:
        B = len(lens)
        q, k, v, g = (torch.randn(B, L, H, device=dev, generator=gen) for _ in range(4))
        tl = torch.from_numpy(lens).to(dev)
        add_mask = ((torch.arange(L, device=dev)[None, :] >= tl[:, None]).float() * -10000.0)[:, None, None, :]
        data.append((q, k, v, g, add_mask, tl))
    pairs = sum(float((lens.astype("float64") ** 2).sum()) for _, lens in calls)
    flop_fwd, flop_bwd = 2 * 2 * 64 * N_HEADS * pairs, 5 * 2 * 64 * N_HEADS * pairs

    def forward_only(fn):
        def run():
            with torch.no_grad():
                for q, k, v, g, m, tl in data:
                    fn(q, k, v, m, tl, True)
        return run

    def forward_backward(fn):
        def run():
            for q, k, v, g, m, tl in data:
                q, k, v = (t.detach().requires_grad_(True) for t in (q, k, v))
                fn(q, k, v, m, tl, True).backward(g)
        return run

    variants, dropped = dict(VARIANTS), {}
    try:
        forward_backward(sdpa)()
        torch.cuda.synchronize()
    except RuntimeError as e:  # pragma: no cover - the yardstick depends on the torch build; the other two never fall back
        dropped["sdpa"] = repr(e)[:300]
        del variants["sdpa"]
    seen = {v: dict(fwd=[], fwdbwd=[]) for v in variants}
    for _ in range(rounds):
        for vname, fn in variants.items():
            seen[vname]["fwd"].append(time_calls(forward_only(fn), steps, warmup))
            seen[vname]["fwdbwd"].append(time_calls(forward_backward(fn), steps, warmup))
        print(name, "round", {k: round(v["fwdbwd"][-1], 4) for k, v in seen.items()}, flush=True)
    res = dict(tower_calls=[dict(B=len(lens), L=L, valid_rows=int(lens.sum()), lens=[int(x) for x in lens]) for L, lens in calls],
               algorithm_gflop=dict(forward=round(flop_fwd / 1e9, 3), backward=round(flop_bwd / 1e9, 3)), variants={},
               variants_unavailable=dropped)
    for vname, fn in variants.items():
        r = {}
        for leg in ("fwd", "fwdbwd"):
            xs = seen[vname][leg]
            r[leg + "_ms"] = dict(median=round(statistics.median(xs), 4), rounds=[round(x, 4) for x in xs], spread=round(max(xs) - min(xs), 4))
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        forward_backward(fn)()
        torch.cuda.synchronize()
        r["peak_bytes_over_the_pair"] = int(torch.cuda.max_memory_allocated() - base)
        if trace:
            try:
                r["traced_launches_fwdbwd"] = traced_launches(forward_backward(fn))
            except Exception as e:  # pragma: no cover - depends on the profiler of the torch build
                r["traced_launches_fwdbwd"] = dict(unavailable=repr(e))
        res["variants"][vname] = r
    f, e = res["variants"]["fused"], res["variants"]["eager"]
    f["share_of_fp32_matrix_peak"] = dict(
        forward=round(flop_fwd / (f["fwd_ms"]["median"] * 1e-3) / PEAK_F32_MATRIX, 4),
        forward_backward=round((flop_fwd + flop_bwd) / (f["fwdbwd_ms"]["median"] * 1e-3) / PEAK_F32_MATRIX, 4),
        basis="algorithm FLOP over the valid rows (2 + 5 products) / event time of the whole call sequence / 157.3e12")
    gain = e["fwdbwd_ms"]["median"] - f["fwdbwd_ms"]["median"]
    res["eager_minus_fused_fwdbwd_ms"] = round(gain, 4)
    res["fused_faster_than_eager_by_more_than_the_spread"] = bool(gain > max(e["fwdbwd_ms"]["spread"], f["fwdbwd_ms"]["spread"]))
    res["fused_peak_memory_lower_than_eager"] = bool(f["peak_bytes_over_the_pair"] < e["peak_bytes_over_the_pair"])
    res["eager_over_fused_fwdbwd"] = round(e["fwdbwd_ms"]["median"] / f["fwdbwd_ms"]["median"], 3)
    return res


def kernel_resources():
    """Registers, LDS and scratch of every kernel of csrc/attention_train.hip, from the compiler's own resource report."""
    import re
    import subprocess
    import tempfile
    src = os.path.join(ROOT, "ance_amd", "csrc", "attention_train.hip")
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                            "-o", os.path.join(tmp, "x.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True)
    out, cur = {}, None
    keys = {"VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane", "LDS Size [bytes/block]": "lds_bytes",
            "Occupancy [waves/SIMD]": "waves_per_simd", "SGPRs": "sgprs"}
    for line in r.stdout.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], stdout=subprocess.PIPE, text=True).stdout.strip() or m.group(1)
            cur = out.setdefault(re.sub(r"\(anonymous namespace\)::|\(.*$|ance::|void ", "", name), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+(?:\[[^\]]+\])?): (\d+)", line)
        if m and cur is not None and m.group(1).strip() in keys:
            cur[keys[m.group(1).strip()]] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="warmup,firstp,maxp,dpr")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--resources-only", action="store_true", help="write only the compiler's resource report of the kernels (no GPU needed)")
    ap.add_argument("--resources-from", default=None, help="a JSON written with --resources-only, merged into the output")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_attention_train.json"))
    a = ap.parse_args()
    if a.resources_only:
        with open(a.out, "w") as f:
            json.dump(kernel_resources(), f, indent=1)
        return
    import torch
    assert torch.cuda.is_available(), "bench_attention_train.py times the GPU; there is no CPU measurement"
    from ance_amd import attention
    attention.manual_seed(0)
    out = dict(what="self-attention core of one encoder layer, forward and forward + backward, fp32, 12 heads, attention dropout 0.1, "
                    "training mode; the step's tower calls back to back",
               device=torch.cuda.get_device_name(0), torch=torch.__version__,
               timing=dict(rounds=a.rounds, calls_per_window=a.steps, warmup_calls=a.warmup))
    if a.resources_from:
        with open(a.resources_from) as f:
            out["kernel_resources_from_the_compiler_report"] = json.load(f)
    all_shapes = shapes()
    for name in a.shapes.split(","):
        out[name] = bench(name, all_shapes[name], a.rounds, a.steps, a.warmup, not a.no_trace)
        print(name, json.dumps({k: v for k, v in out[name].items() if k != "tower_calls"}), flush=True)
        torch.cuda.empty_cache()
    if a.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
