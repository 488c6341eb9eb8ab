"""Times one AdamW optimizer step over RobertaDot_NLL_LN's parameters (RoBERTa-base and -large shapes, tests/lamb_util.py, grouped as
drivers/run_ann.py:58-78 does; the classifier tensors present without gradients) with device events, in ONE process, the variants
alternated --rounds times (each round times every variant once: --steps steps after --warmup):
  (1) fused        ance_amd.optim.AdamW.step()                      -> ance_adamw_step (csrc/adamw.hip), 28 B of HBM traffic per element
  (2) torch_fused  torch.optim.AdamW(fused=True).step()             a vendor yardstick of the same traffic (28 B; another arithmetic)
  (3) loop         the transformers 2.3.0 step as a per-tensor torch loop, the form the reference runs
  (4) fused_clip   AdamW(max_grad_norm=1.0).step()                  -> 32 B per element
      torch_clip   torch.nn.utils.clip_grad_norm_(params, 1.0); (2)  -> 44 B per element (norm 4, rescale 8 + 4, step 28)
Beside the times: achieved bytes per second at 28 / 32 B per element, the ratio to the byte floor at the bandwidth
profiles/r07_lamb_step.json shows the LAMB step reaching at that size, the kernel launches per call traced with torch.profiler
(after the timing, a region of --trace-calls calls and nothing else), and the max |delta| of a seeded sample of every tensor from
the fp64 restatement (tests/adamw_util.py) after the first fused step, and the host time to enqueue one call of each variant
(a window of --steps calls with no synchronise inside).  Writes one JSON object (--out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BYTES = {"fused": 28, "torch_fused": 28, "loop": 28, "fused_clip": 32, "torch_clip": 44}  # loop: the algorithm's floor, not its traffic
LR, EPS, WD, BETAS = 1e-4, 1e-6, 0.01, (0.9, 0.999)
SAMPLE = 4096


def time_steps(fn, steps, warmup):
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


def host_ms_per_call(fn, calls):
    """Host time to enqueue one call (no synchronise inside the window): where it reaches the step's time, the host bounds the step."""
    import time
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) / calls * 1e3


def loop_step(params, state, lr=LR, betas=BETAS, eps=EPS, wd=WD):
    """transformers 2.3.0 optimization.py AdamW.step, restated per tensor."""
    import math
    b1, b2 = betas
    for p in params:
        if p.grad is None:
            continue
        st = state.setdefault(p, {})
        if not st:
            st["step"], st["m"], st["v"] = 0, p.data.new_zeros(p.shape), p.data.new_zeros(p.shape)
        m, v = st["m"], st["v"]
        st["step"] += 1
        m.mul_(b1).add_(p.grad, alpha=1.0 - b1)
        v.mul_(b2).addcmul_(p.grad, p.grad, value=1.0 - b2)
        denom = v.sqrt().add_(eps)
        ss = lr * math.sqrt(1.0 - b2 ** st["step"]) / (1.0 - b1 ** st["step"])
        p.data.addcdiv_(m, denom, value=-ss)
        if wd > 0.0:
            p.data.add_(p.data, alpha=-lr * wd)


def traced_launches(fn, calls):
    """Kernel launches per call: a torch.profiler region of `calls` calls and nothing else on the GPU."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    kernels, copies = {}, 0
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            if "memcpy" in e.name.lower() or "memset" in e.name.lower():
                copies += 1
            elif not e.name.startswith("Optimizer.step"):   # the profiler's own annotation of the region is no launch
                kernels[e.name[:90]] = kernels.get(e.name[:90], 0) + 1
    return dict(kernels_per_call=round(sum(kernels.values()) / calls, 2), copies_per_call=round(copies / calls, 2),
                by_name={k: round(v / calls, 2) for k, v in sorted(kernels.items())})


def bench(kind, rounds, steps, warmup, trace_calls, lamb_tb_s):
    import numpy as np
    import torch
    import adamw_util as W
    import lamb_util as U
    from ance_amd.optim import AdamW
    dev = torch.device("cuda:0")
    host = U.roberta_param_groups(kind)
    print(kind, "parameters generated", flush=True)

    def build(seed=0):
        gen = torch.Generator(device=dev).manual_seed(seed)   # the same gradients for every variant
        groups, n = [], 0
        for gname, plist in host:
            ps = []
            for name, t, has_grad in plist:
                p = torch.nn.Parameter(t.to(dev))
                if has_grad:
                    p.grad = torch.randn(t.shape, device=dev, generator=gen) * 1e-3
                    n += p.numel()
                ps.append(p)
            groups.append(dict(params=ps))
        return groups, n

    sets = {name: build() for name in BYTES}
    n = sets["fused"][1]
    flat = {name: [p for g in sets[name][0] for p in g["params"]] for name in sets}
    opt = {"fused": AdamW(sets["fused"][0], lr=LR, eps=EPS, weight_decay=WD),
           "fused_clip": AdamW(sets["fused_clip"][0], lr=LR, eps=EPS, weight_decay=WD, max_grad_norm=1.0),
           "torch_fused": torch.optim.AdamW(sets["torch_fused"][0], lr=LR, eps=EPS, weight_decay=WD, fused=True),
           "torch_clip": torch.optim.AdamW(sets["torch_clip"][0], lr=LR, eps=EPS, weight_decay=WD, fused=True)}
    loop_state = {}

    def torch_clip():
        # clip_grad_norm_ rescales p.grad in memory, so from the second call on the norm is at most 1: torch still reads every
        # gradient for the norm and multiplies every gradient by the clamped factor, which is a training step's traffic
        torch.nn.utils.clip_grad_norm_(flat["torch_clip"], 1.0)
        opt["torch_clip"].step()

    legs = {"fused": opt["fused"].step, "torch_fused": opt["torch_fused"].step, "loop": lambda: loop_step(flat["loop"], loop_state),
            "fused_clip": opt["fused_clip"].step, "torch_clip": torch_clip}

    # accuracy of the first fused step on a seeded sample of every tensor, before anything else steps that set
    rng = np.random.default_rng(11)
    sample = []
    for gi, g in enumerate(sets["fused"][0]):
        for p in g["params"]:
            if p.grad is None:
                continue
            ix = torch.from_numpy(np.sort(rng.choice(p.numel(), size=min(SAMPLE, p.numel()), replace=False))).to(dev)
            sample.append((p, ix, p.detach().view(-1)[ix].cpu().numpy(), p.grad.view(-1)[ix].cpu().numpy()))
    opt["fused"].step()
    torch.cuda.synchronize()
    worst = dict(p=0.0, m=0.0, v=0.0, p_ulp=0.0)
    for p, ix, p0, g0 in sample:
        st = opt["fused"].state[p]
        want = W.step_fp64(p0, g0, np.zeros_like(p0, np.float64), np.zeros_like(p0, np.float64), 1, LR, BETAS, EPS, WD, True)
        got = (p.detach().view(-1)[ix], st["exp_avg"].view(-1)[ix], st["exp_avg_sq"].view(-1)[ix])
        for key, a, b in zip("pmv", got, want):
            worst[key] = max(worst[key], float(np.abs(a.cpu().numpy().astype(np.float64) - b).max()))
        d = np.abs(got[0].cpu().numpy().astype(np.float64) - want[0]).max() / U.ulp32(np.abs(want[0]).max())
        worst["p_ulp"] = max(worst["p_ulp"], float(d))
    print(kind, "sampled max |delta| to fp64", json.dumps(worst), flush=True)

    seen = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            seen[name].append(time_steps(fn, steps, warmup))
        print(kind, "round", {k: round(v[-1], 4) for k, v in seen.items()}, flush=True)
    res = dict(n_tensors_with_grad=len(sample), n_elements_with_grad=n, lamb_achieved_tb_s=lamb_tb_s, legs={},
               sampled_max_abs_delta_to_fp64_after_step_1=dict(elements_per_tensor=SAMPLE, **{k: float("%.3g" % v) for k, v in worst.items()}))
    for name, v in seen.items():
        med = statistics.median(v)
        byts = BYTES[name] * n
        res["legs"][name] = dict(median_ms=round(med, 4), rounds_ms=[round(x, 4) for x in v], spread_ms=round(max(v) - min(v), 4),
                                 bytes_per_element=BYTES[name], achieved_tb_s=round(byts / (med * 1e-3) / 1e12, 3))
        res["legs"][name]["host_enqueue_ms_per_call"] = round(host_ms_per_call(legs[name], steps), 4)
        if lamb_tb_s:
            floor = byts / (lamb_tb_s * 1e12) * 1e3
            res["legs"][name].update(floor_ms_at_lamb_rate=round(floor, 4), time_over_floor=round(med / floor, 3))
    L = res["legs"]
    spread = max(L["fused_clip"]["spread_ms"], L["torch_clip"]["spread_ms"])
    res["torch_clip_minus_fused_clip_ms"] = round(L["torch_clip"]["median_ms"] - L["fused_clip"]["median_ms"], 4)
    res["fused_clip_faster_than_torch_clip_by_more_than_the_spread"] = res["torch_clip_minus_fused_clip_ms"] > spread
    res["torch_fused_over_fused"] = round(L["torch_fused"]["median_ms"] / L["fused"]["median_ms"], 3)   # reported, not gated
    res["loop_over_fused"] = round(L["loop"]["median_ms"] / L["fused"]["median_ms"], 2)
    if trace_calls > 0:
        try:
            res["traced_launches"] = {name: traced_launches(fn, trace_calls) for name, fn in legs.items() if name != "loop"}
        except Exception as e:  # pragma: no cover - depends on the profiler of the torch build
            res["traced_launches"] = dict(unavailable=repr(e))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="base,large")
    ap.add_argument("--trace-calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_adamw_step.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_adamw.py times the GPU; there is no CPU measurement"
    lamb = {}
    try:
        with open(os.path.join(ROOT, "profiles", "r07_lamb_step.json")) as f:
            r07 = json.load(f)
        lamb = {k: r07[k]["legs"]["fused"]["achieved_tb_s"] for k in ("base", "large") if k in r07}
    except OSError:
        pass
    out = dict(what="one AdamW optimizer step (transformers 2.3.0 arithmetic), RobertaDot_NLL_LN parameters, run_ann.py grouping",
               device=torch.cuda.get_device_name(0), torch=torch.__version__, rounds=a.rounds, steps=a.steps, warmup=a.warmup,
               hyper_parameters=dict(lr=LR, eps=EPS, weight_decay=WD, betas=list(BETAS), max_grad_norm=1.0),
               floor_basis="bytes per element at the rate profiles/r07_lamb_step.json shows the fused LAMB step reaching")
    for kind in a.sizes.split(","):
        out[kind] = bench(kind, a.rounds, a.steps, a.warmup, a.trace_calls, lamb.get(kind))
        print(kind, json.dumps(out[kind]), flush=True)
        torch.cuda.empty_cache()
    if a.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
