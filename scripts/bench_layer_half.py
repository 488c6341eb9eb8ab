"""Times forward + backward of ONE BertLayer under torch.autocast(fp16), training mode, dropout 0.1, all sequences full, in ONE
process with the three variants alternated --rounds times (every round kept):
  eager        transformers 2.3.0's BertLayer restated in eager torch (bench_layer_tail.EagerBertLayer)
  half_attn    ance_amd.layers.BertLayer(attention_precision="half"): the 16-bit attention core, fp32 seams (the casts around them)
  half         ance_amd.layers.BertLayer(precision="half"): 16-bit seams as well, fp32 residual stream, one activation cast
Shapes: 8 x 512 and 32 x 128 rows, hidden 768 (12 heads, FFN 3072) and 1024 (16 heads, FFN 4096).
Per variant: the device-event median of every round and their median and spread, the host time to enqueue one forward + backward
(time.perf_counter around a window of calls that nothing synchronises), the launches and the summed device time of one traced forward
+ backward, and torch.cuda.max_memory_allocated over one forward + backward above what was allocated before it.  No speed-up is fixed
in advance: the yardstick of `half` is `half_attn` in the same process, and the ratio is reported at every shape, whichever way it
falls.  Where the host enqueue time is not below the event time the shape is host-bound and the device times say what the GPU spends.
Writes one JSON object (--out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_layer_tail as BT  # noqa: E402

P_DROP = BT.P_DROP


def host_enqueue_ms(fn, steps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) * 1e3 / steps


def bench_shape(B, L, hidden, rounds, steps, warmup):
    import torch
    from ance_amd.layers import BertLayer
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    heads, inter = BT.WIDTHS[hidden]
    base = BertLayer(hidden, heads, inter, 1e-5, P_DROP, P_DROP).to(dev).train()
    layers = dict(half_attn=BertLayer(hidden, heads, inter, 1e-5, P_DROP, P_DROP, attention_precision="half").to(dev).train(),
                  half=BertLayer(hidden, heads, inter, 1e-5, P_DROP, P_DROP, precision="half").to(dev).train())
    for m in layers.values():
        m.load_state_dict(base.state_dict())
    eager = BT.EagerBertLayer(base)
    hs = torch.randn(B, L, hidden, device=dev, generator=gen)
    dout = torch.randn(B, L, hidden, device=dev, generator=gen)
    lens = torch.full((B,), L, dtype=torch.int32, device=dev)
    add_mask = torch.zeros(B, 1, 1, L, device=dev)

    def run_eager():
        a = hs.detach().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16):
            out = eager(a, add_mask)
        out.float().backward(dout)
        base.zero_grad(set_to_none=True)

    def run(m):
        def fn():
            a = hs.detach().requires_grad_(True)
            with torch.autocast("cuda", dtype=torch.float16):
                out = m(a, lens)
            out.float().backward(dout)
            m.zero_grad(set_to_none=True)
        return fn

    variants = dict(eager=run_eager, half_attn=run(layers["half_attn"]), half=run(layers["half"]))
    tag = "layer %dx%d H%d" % (B, L, hidden)
    seen, host = {v: [] for v in variants}, {v: [] for v in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            seen[name].append(BT.time_calls(fn, steps, warmup))
            host[name].append(host_enqueue_ms(fn, steps))
        print(tag, "round", {k: round(v[-1], 4) for k, v in seen.items()}, flush=True)
    out = {}
    for name, fn in variants.items():
        xs = seen[name]
        out[name] = dict(fwdbwd_ms=dict(median=round(statistics.median(xs), 4), rounds=[round(x, 4) for x in xs], spread=round(max(xs) - min(xs), 4)),
                         host_enqueue_ms=dict(median=round(statistics.median(host[name]), 4), rounds=[round(x, 4) for x in host[name]]),
                         peak_bytes_over_the_pair=BT.peak_bytes(fn))
        try:
            out[name]["traced_fwdbwd"] = BT.traced(fn)
        except Exception as e:  # pragma: no cover - depends on the profiler of the torch build
            out[name]["traced_fwdbwd"] = dict(unavailable=repr(e))
        out[name]["host_bound"] = bool(out[name]["host_enqueue_ms"]["median"] >= 0.9 * out[name]["fwdbwd_ms"]["median"])
    a, h = out["half_attn"], out["half"]
    res = dict(variants=out,
               half_attn_over_half_fwdbwd=round(a["fwdbwd_ms"]["median"] / h["fwdbwd_ms"]["median"], 3),
               eager_over_half_fwdbwd=round(out["eager"]["fwdbwd_ms"]["median"] / h["fwdbwd_ms"]["median"], 3),
               half_faster_than_half_attn_by_more_than_the_spread=bool(
                   a["fwdbwd_ms"]["median"] - h["fwdbwd_ms"]["median"] > max(a["fwdbwd_ms"]["spread"], h["fwdbwd_ms"]["spread"])),
               half_peak_memory_over_half_attn=round(h["peak_bytes_over_the_pair"] / a["peak_bytes_over_the_pair"], 3))
    if "device_time_us" in a["traced_fwdbwd"] and "device_time_us" in h["traced_fwdbwd"]:
        res["half_attn_over_half_device_time"] = round(a["traced_fwdbwd"]["device_time_us"] / h["traced_fwdbwd"]["device_time_us"], 3)
        res["launches_half_attn_minus_half"] = a["traced_fwdbwd"]["kernels"] - h["traced_fwdbwd"]["kernels"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_layer_half.json"))
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5: every round is kept and the median is over them")
    import torch
    assert torch.cuda.is_available(), "bench_layer_half.py times the GPU; there is no CPU measurement"
    from ance_amd import attention
    attention.manual_seed(0)
    out = dict(what="one BertLayer, forward + backward under torch.autocast(fp16), training mode, dropout 0.1, all sequences full: eager "
                    "torch, BertLayer(attention_precision=\"half\") and BertLayer(precision=\"half\"), alternated in one process",
               device=torch.cuda.get_device_name(0), torch=torch.__version__,
               timing=dict(rounds=a.rounds, calls_per_window=a.steps, warmup_calls=a.warmup))
    for sname, (B, L) in BT.SHAPES.items():
        for hidden in BT.WIDTHS:
            key = "%s_h%d" % (sname, hidden)
            out[key] = bench_shape(B, L, hidden, a.rounds, a.steps, a.warmup)
            print(key, json.dumps(out[key]), flush=True)
            torch.cuda.empty_cache()
    if a.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
