"""Times the self-attention core under the reference's --fp16 recipe -- torch.autocast("cuda", dtype=torch.float16), fp16 Linear
outputs going in -- with device events, in ONE process, the variants alternated --rounds times:
  (a) half    attention_padded(..., precision="half") -> csrc/attention_train_half.hip: fp16 in and out
  (b) fp32    attention_padded(...) as autocast drives the default: the three fp16 inputs cast to fp32, the fp32 core, an fp32 ctx
              cast down again for the next F.linear, and the reverse casts in the backward
  (c) sdpa    torch.nn.functional.scaled_dot_product_attention on the fp16 tensors with the additive mask and dropout: a yardstick
Shapes, timing windows, peak memory and traced launches are those of scripts/bench_attention_train.py (the step's tower calls back to
back, training mode, attention dropout 0.1).  Every variant hands an fp16 ctx to the next layer and receives an fp16 gradient.
Writes one JSON object (--out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import bench_attention_train as B32  # noqa: E402

N_HEADS, H, P_DROP = B32.N_HEADS, B32.H, B32.P_DROP


def half(q, k, v, add_mask, lens, training):
    from ance_amd.attention import attention_padded
    return attention_padded(q, k, v, lens, N_HEADS, P_DROP, training, precision="half")


def fp32(q, k, v, add_mask, lens, training):
    from ance_amd.attention import attention_padded
    return attention_padded(q, k, v, lens, N_HEADS, P_DROP, training).half()   # what the next F.linear does under autocast


def sdpa(q, k, v, add_mask, lens, training):
    return B32.sdpa(q, k, v, add_mask.half(), lens, training)


VARIANTS = {"half": half, "fp32": fp32, "sdpa": sdpa}


def bench(name, calls, rounds, steps, warmup, trace):
    import torch
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    data = []
    for L, lens in calls:
        q, k, v, g = (torch.randn(len(lens), L, H, device=dev, generator=gen).half() for _ in range(4))
        tl = torch.from_numpy(lens).to(dev)
        add_mask = ((torch.arange(L, device=dev)[None, :] >= tl[:, None]).float() * -10000.0)[:, None, None, :]
        data.append((q, k, v, g, add_mask, tl))

    def forward_only(fn):
        def run():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                for q, k, v, g, m, tl in data:
                    fn(q, k, v, m, tl, True)
        return run

    def forward_backward(fn):
        def run():
            for q, k, v, g, m, tl in data:
                q, k, v = (t.detach().requires_grad_(True) for t in (q, k, v))
                with torch.autocast("cuda", dtype=torch.float16):
                    out = fn(q, k, v, m, tl, True)
                out.backward(g)
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
            seen[vname]["fwd"].append(B32.time_calls(forward_only(fn), steps, warmup))
            seen[vname]["fwdbwd"].append(B32.time_calls(forward_backward(fn), steps, warmup))
        print(name, "round", {k: round(v["fwdbwd"][-1], 4) for k, v in seen.items()}, flush=True)
    res = dict(tower_calls=[dict(B=len(lens), L=L, valid_rows=int(lens.sum())) for L, lens in calls], variants={}, variants_unavailable=dropped)
    for vname, fn in variants.items():
        r = {}
        for leg in ("fwd", "fwdbwd"):
            xs = seen[vname][leg]
            # best: where the host, not the device, sets a window's time (half and sdpa at every shape here), a busy host shows as
            # whole rounds at up to twice the time of the others; the device-bound fp32 variant does not move
            r[leg + "_ms"] = dict(median=round(statistics.median(xs), 4), best=round(min(xs), 4), rounds=[round(x, 4) for x in xs],
                                  spread=round(max(xs) - min(xs), 4))
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        forward_backward(fn)()
        torch.cuda.synchronize()
        r["peak_bytes_over_the_pair"] = int(torch.cuda.max_memory_allocated() - base)
        if trace:
            try:
                r["traced_launches_fwdbwd"] = B32.traced_launches(forward_backward(fn))
            except Exception as e:  # pragma: no cover - depends on the profiler of the torch build
                r["traced_launches_fwdbwd"] = dict(unavailable=repr(e))
        res["variants"][vname] = r
    a, b = res["variants"]["half"], res["variants"]["fp32"]
    gain = b["fwdbwd_ms"]["median"] - a["fwdbwd_ms"]["median"]
    res["fp32_over_half_fwd"] = round(b["fwd_ms"]["median"] / a["fwd_ms"]["median"], 3)
    res["fp32_over_half_fwdbwd"] = round(b["fwdbwd_ms"]["median"] / a["fwdbwd_ms"]["median"], 3)
    res["half_faster_than_fp32_by_more_than_the_spread"] = bool(gain > max(a["fwdbwd_ms"]["spread"], b["fwdbwd_ms"]["spread"]))
    res["half_peak_memory_lower_than_fp32"] = bool(a["peak_bytes_over_the_pair"] < b["peak_bytes_over_the_pair"])
    if "sdpa" in res["variants"]:
        c = res["variants"]["sdpa"]
        res["sdpa_over_half_fwd"] = round(c["fwd_ms"]["median"] / a["fwd_ms"]["median"], 3)
        res["sdpa_over_half_fwdbwd"] = round(c["fwdbwd_ms"]["median"] / a["fwdbwd_ms"]["median"], 3)
    return res


def kernel_device_times(calls, reps=10):
    """Mean device time (us) of every attention kernel, from torch.profiler, at the largest tower call of `calls`: precision="half"
    in fp16 and the fp32 core, each with dropout 0.1 and without -- what the dropout stream costs inside the loop, and how the kernels
    themselves compare where the event times above are set by the host."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    from ance_amd.attention import attention_padded
    dev = torch.device("cuda:0")
    L, lens = max(calls, key=lambda c: int(c[1].sum()))
    tl = torch.from_numpy(lens).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    q, k, v, g = (torch.randn(len(lens), L, H, device=dev, generator=gen) for _ in range(4))
    out = dict(call=dict(B=len(lens), L=L, valid_rows=int(lens.sum())))
    for name, dt, prec in (("half", torch.float16, "half"), ("fp32", torch.float32, "fp32")):
        for p in (P_DROP, 0.0):
            def run():
                a, b, c = (t.to(dt).requires_grad_(True) for t in (q, k, v))
                attention_padded(a, b, c, tl, N_HEADS, p, True, precision=prec).backward(g.to(dt))
            for _ in range(3):
                run()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(reps):
                    run()
                torch.cuda.synchronize()
            rows = {}
            for e in prof.key_averages():
                for kern in ("fwd", "rowdot", "dkv", "dq"):
                    if "attn" in e.key and "_%s_kernel" % kern in e.key:
                        rows[kern] = round(e.device_time_total / e.count, 2)
            rows["sum"] = round(sum(rows.values()), 2)
            out["%s, dropout %g" % (name, p)] = rows
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="warmup,firstp,maxp,dpr")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_attention_half.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_attention_half.py times the GPU; there is no CPU measurement"
    from ance_amd import attention
    attention.manual_seed(0)
    out = dict(what="self-attention core of one encoder layer under torch.autocast(fp16): forward and forward + backward, fp16 inputs and "
                    "gradients, 12 heads, attention dropout 0.1, training mode; the step's tower calls back to back",
               variants=dict(half="precision=\"half\"", fp32="the default under autocast: casts to fp32 and back included",
                             sdpa="scaled_dot_product_attention on the fp16 tensors"),
               device=torch.cuda.get_device_name(0), torch=torch.__version__,
               timing=dict(rounds=a.rounds, calls_per_window=a.steps, warmup_calls=a.warmup))
    all_shapes = B32.shapes()
    for name in a.shapes.split(","):
        out[name] = bench(name, all_shapes[name], a.rounds, a.steps, a.warmup, not a.no_trace)
        print(name, json.dumps({k: v for k, v in out[name].items() if k != "tower_calls"}), flush=True)
        torch.cuda.empty_cache()
    if not a.no_trace:
        try:
            out["kernel_device_time_us_firstp_documents"] = kernel_device_times(all_shapes["firstp"])
        except Exception as e:  # pragma: no cover - depends on the profiler of the torch build
            out["kernel_device_time_us_firstp_documents"] = dict(unavailable=repr(e))
        print("kernels", json.dumps(out["kernel_device_time_us_firstp_documents"]), flush=True)
    if a.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
