"""Times a WHOLE training step -- three tower calls, the triplet objective, the backward, Lamb(max_grad_norm=1.0), the linear warm-up
schedule -- three ways, in ONE process, the variants alternated --rounds times and every round kept:
  (a) eager_host    the step as before this feature: the dropout stream in host mode, a float lr that transformers'
                    get_linear_schedule_with_warmup changes after every step (so the optimizer's tables are rebuilt and uploaded at
                    every step, as they always were)
  (b) eager_device  the same step eagerly with dropout_state.to_device(), the resident plan and LinearWarmupSchedule (a device lr)
  (c) graph_replay  (b) captured once by the recipe of INTEGRATION.md and replayed
The tower is 12 layers of BertEmbeddings / BertLayer and a head (tests/train_step_util.py's device_tower at RoBERTa-base width, seeded
weights), dropout 0.1, at the README's shapes: B x (Lq, Ld, Ld) = 8 x (64, 512, 512) and 32 x (64, 128, 128); fp32, and under
torch.autocast(fp16) with precision="half" (no GradScaler: capturing the scaler is outside this feature, so the fp16 rows time the
step's launches, not a usable loss scale).  Per variant: host wall time per step (a window of steps with one synchronise behind
it), device time per step (events around the window), and the kernel launches and copies of one traced step.  (torch.profiler
sees a replayed graph as one graph launch, not as its kernels: the traced counts of graph_replay are 0 and 0.)

Separately, the optimizer step alone over RoBERTa-base's 201 tensors (tests/lamb_util.py's roberta_param_groups, as
scripts/bench_adamw.py / bench_lamb.py build them): the first step (state and plan are built), a later step with the resident plan,
and a step behind invalidate_plan() (the tables rebuilt and uploaded: what every step did before), next to what the parent's
profiles/r09_adamw_step.json and r07_lamb_step.json hold.  No speed-up is asserted anywhere: the JSON holds what was measured."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"8x(64,512,512)": (8, (64, 512, 512)), "32x(64,128,128)": (32, (64, 128, 128))}
CFG = dict(H=768, heads=12, inter=3072, N=12, mode="absolute", n_types=2, eps=1e-5, pad=0)
WARM, TOTAL = 10, 100000


def traced(fn):
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    kernels, copies = 0, 0
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            if "memcpy" in e.name.lower() or "memset" in e.name.lower():
                copies += 1
            elif not e.name.startswith("Optimizer.step"):
                kernels += 1
    return dict(kernel_launches=kernels, copies=copies)


def window(fn, steps):
    """(host ms per step to enqueue, wall ms per step with the synchronise, device ms per step between two events)."""
    import torch
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t1 - t0) / steps * 1e3, (t2 - t0) / steps * 1e3, a.elapsed_time(b) / steps


def rounds_of(windows, k):
    """Entry k of every round's window: the median and every round."""
    return dict(median=round(statistics.median(x[k] for x in windows), 4), rounds=[round(x[k], 4) for x in windows])


def batches(B, lens3, vocab, gen):
    import torch
    out = []
    for L in lens3:
        ids = torch.randint(1, vocab, (B, L), device="cuda:0", generator=gen)
        lens = torch.randint(max(1, L // 2), L + 1, (B,), device="cuda:0", generator=gen, dtype=torch.int32)
        ids[torch.arange(L, device="cuda:0")[None, :] >= lens[:, None]] = 0
        out.append((ids, torch.zeros_like(ids), lens))
    return out


def make_variant(name, sd, B, lens3, half):
    """A closure that runs one step of variant `name` on its own tower, optimizer and schedule."""
    import torch
    import lamb_util as U
    import train_step_util as S
    from transformers import get_linear_schedule_with_warmup
    from ance_amd import attention as T
    from ance_amd.loss import nll_loss
    from ance_amd.optim import Lamb, LinearWarmupSchedule
    tower = S.device_tower(CFG, sd, 0.1, precision="half" if half else "fp32").train()
    opt = Lamb(S.param_groups(tower), lr=1e-3, betas=U.BETAS, eps=U.EPS, max_grad_norm=1.0)
    gen = torch.Generator(device="cuda:0").manual_seed(5)
    static = batches(B, lens3, S.VOCAB, gen)
    device_mode = name != "eager_host"
    sched = LinearWarmupSchedule(opt, WARM, TOTAL) if device_mode else get_linear_schedule_with_warmup(opt, WARM, TOTAL)

    def step():
        with torch.autocast("cuda", dtype=torch.float16, enabled=half):
            loss = nll_loss(*[tower(*c) for c in static])
        loss.backward()
        opt.step()
        sched.step()
        if device_mode:
            T.dropout_state.advance(0)

    def eager():
        step()
        opt.zero_grad(set_to_none=True)

    def enter():   # the dropout stream is one object for the process: each variant switches it to its mode when its turn comes
        if device_mode:
            T.dropout_state.to_device(0)
        else:
            T.dropout_state.to_host(0)

    if name != "graph_replay":
        return enter, eager
    enter()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            eager()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    return enter, graph.replay


def bench_steps(rounds, steps, warmup):
    import torch
    import train_step_util as S
    sd = S.tower_state(CFG)
    res = {}
    for half in (False, True):
        for shape, (B, lens3) in SHAPES.items():
            key = "%s %s" % ("autocast_fp16_half" if half else "fp32", shape)
            legs = {name: make_variant(name, sd, B, lens3, half) for name in ("eager_host", "eager_device", "graph_replay")}
            seen = {name: [] for name in legs}
            for _ in range(rounds):
                for name, (enter, fn) in legs.items():
                    enter()
                    for _ in range(warmup):
                        fn()
                    seen[name].append(window(fn, steps))
                print(key, "round", {k: [round(x, 3) for x in v[-1]] for k, v in seen.items()}, flush=True)
            out = {}
            for name, (enter, fn) in legs.items():
                enter()
                v = seen[name]
                out[name] = dict(host_enqueue_ms_per_step=rounds_of(v, 0), wall_ms_per_step=rounds_of(v, 1),
                                 device_event_ms_per_step=rounds_of(v, 2), traced_step=traced(fn))
            res[key] = out
            del legs
            torch.cuda.empty_cache()
    return res


def bench_optimizer(rounds, steps, warmup):
    """The optimizer step alone, RoBERTa-base's 201 tensors: first step, resident plan, rebuilt plan."""
    import torch
    import lamb_util as U
    from ance_amd.optim import AdamW, Lamb
    dev = torch.device("cuda:0")
    host = U.roberta_param_groups("base")
    res = {}
    for kind, Opt in (("lamb_clip", Lamb), ("adamw_clip", AdamW)):
        gen = torch.Generator(device=dev).manual_seed(0)
        groups = []
        for _, plist in host:
            ps = []
            for _, t, has_grad in plist:
                p = torch.nn.Parameter(t.to(dev))
                if has_grad:
                    p.grad = torch.randn(t.shape, device=dev, generator=gen) * 1e-3
                ps.append(p)
            groups.append(dict(params=ps))
        opt = Opt(groups, lr=1e-4, eps=1e-6, weight_decay=0.01, max_grad_norm=1.0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.step()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        first = dict(host_enqueue_ms=round((t1 - t0) * 1e3, 4), wall_ms=round((time.perf_counter() - t0) * 1e3, 4))

        def rebuilt():
            opt.invalidate_plan()
            opt.step()

        legs = dict(resident_plan=opt.step, rebuilt_every_step=rebuilt)
        seen = {name: [] for name in legs}
        for _ in range(rounds):
            for name, fn in legs.items():
                for _ in range(warmup):
                    fn()
                seen[name].append(window(fn, steps))
        out = dict(first_step=first, n_tensors_with_grad=sum(1 for g in groups for p in g["params"] if p.grad is not None))
        for name, fn in legs.items():
            v = seen[name]
            out[name] = dict(host_enqueue_ms_per_step=rounds_of(v, 0), device_event_ms_per_step=rounds_of(v, 2), traced_step=traced(fn))
        res[kind] = out
        del opt, groups
        torch.cuda.empty_cache()
    parent = {}
    for kind, path, leg in (("adamw_clip", "r09_adamw_step.json", "fused_clip"), ("lamb_clip", "r07_lamb_step.json", "fused_clip")):
        try:
            with open(os.path.join(ROOT, "profiles", path)) as f:
                legs = json.load(f)["base"]["legs"]
            parent[kind] = dict(file="profiles/" + path, leg=leg if leg in legs else "fused", **{
                k: legs[leg if leg in legs else "fused"].get(k) for k in ("median_ms", "rounds_ms", "host_enqueue_ms_per_call")})
        except (OSError, KeyError, ValueError) as e:
            parent[kind] = dict(unavailable=repr(e))
    res["parent_profiles"] = parent
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_graph_step.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_graph_step.py times the GPU; there is no CPU measurement"
    assert a.rounds >= 5, "at least five rounds, every round kept"
    out = dict(what="a whole training step (12-layer tower x 3 calls, triplet objective, backward, Lamb(max_grad_norm=1.0), linear warm-up "
                    "schedule, dropout 0.1): eager in host mode, eager with the device stream / resident plan / device lr, and replayed "
                    "from one captured graph; and the optimizer step alone over RoBERTa-base's 201 tensors",
               device=torch.cuda.get_device_name(0), torch=torch.__version__, rounds=a.rounds, steps_per_window=a.steps, warmup=a.warmup,
               note="one process, variants alternated, every round kept; fp16 rows run without a GradScaler")
    out["whole_step"] = bench_steps(a.rounds, a.steps, a.warmup)
    out["optimizer_alone_roberta_base"] = bench_optimizer(a.rounds, 20, 3)
    print(json.dumps(out), flush=True)
    if a.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
