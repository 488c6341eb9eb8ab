"""Times one LAMB optimizer step over RobertaDot_NLL_LN's parameters (RoBERTa-base and -large shapes, grouped as
drivers/run_ann.py:58-78 does; the classifier tensors present without gradients) with device events, median of --steps steps
after --warmup:
  (a) fused    ance_amd.optim.Lamb -> ance_lamb_step (csrc/lamb.hip), 40 B of HBM traffic per element
  (b) loop     the same algorithm as a per-tensor torch loop, the form of the reference's utils/lamb.py (its trust-ratio branch
               and its tensor-valued alpha each wait for the device) -- the stand-in for the reference, which is not on the GPU box
  (c) adamw    torch.optim.AdamW(fused=True) when this torch has it: a vendor yardstick of the same traffic class (28 B per element)
Writes one JSON object (--out).  --kernel-stats DB merges the kernel times of a separate `rocprofv3 --kernel-trace --stats` run
into that file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_ACHIEVABLE, HBM_SPEC = 6.3e12, 8.0e12  # B/s: MI355X float4 copy / datasheet
BYTES_PER_ELEMENT = {"fused": 40, "loop": 40, "adamw": 28}  # loop: the same algorithm's floor (its own traffic is far larger)


def build(kind, dev):
    import torch
    import lamb_util as U
    gen = torch.Generator(device=dev).manual_seed(0)
    groups, n_grad = [], 0
    for gname, plist in U.roberta_param_groups(kind):
        ps = []
        for name, t, has_grad in plist:
            p = torch.nn.Parameter(t.to(dev))
            if has_grad:
                p.grad = torch.randn(t.shape, device=dev, generator=gen) * 1e-3
                n_grad += p.numel()
            ps.append(p)
        groups.append(dict(params=ps))
    return groups, n_grad


def loop_step(groups, state, lr=1e-4, betas=(0.9, 0.999), eps=1e-6, wd=0.0):
    """The reference's per-tensor sequence of torch ops (restated), including its two host waits per tensor."""
    import torch
    b1, b2 = betas
    for g in groups:
        for p in g["params"]:
            if p.grad is None:
                continue
            st = state.setdefault(p, {})
            if not st:
                st["m"], st["v"] = torch.zeros_like(p), torch.zeros_like(p)
            m, v = st["m"], st["v"]
            m.mul_(b1).add_(p.grad, alpha=1 - b1)
            v.mul_(b2).addcmul_(p.grad, p.grad, value=1 - b2)
            wn = p.data.pow(2).sum().sqrt().clamp(0, 10)
            u = m / v.sqrt().add(eps)
            if wd != 0:
                u.add_(p.data, alpha=wd)
            an = u.pow(2).sum().sqrt()
            tr = 1 if (wn == 0 or an == 0) else wn / an
            p.data.add_(u, alpha=float(-lr * tr))


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
    ms = [a.elapsed_time(b) for a, b in ev]
    return statistics.median(ms), min(ms), max(ms)


def bench(kind, steps, warmup, only):
    import torch
    from ance_amd.optim import Lamb
    dev = torch.device("cuda:0")
    groups, n = build(kind, dev)
    n_tensors = sum(1 for g in groups for p in g["params"] if p.grad is not None)
    res = dict(n_tensors=sum(len(g["params"]) for g in groups), n_tensors_with_grad=n_tensors, n_elements_with_grad=n, legs={})
    legs = [("fused", lambda: Lamb(groups, lr=1e-4, eps=1e-6))]
    if only != "fused":
        legs.append(("loop", None))
        legs.append(("adamw", None))
    for name, make in legs:
        if name == "fused":
            opt = make()
            fn = opt.step
        elif name == "loop":
            state = {}
            fn = lambda: loop_step(groups, state)  # noqa: E731
        else:
            try:
                opt = torch.optim.AdamW(groups, lr=1e-4, eps=1e-6, fused=True)
            except Exception as e:  # pragma: no cover - depends on the torch build
                res["legs"][name] = dict(unsupported=str(e))
                continue
            fn = opt.step
        med, lo, hi = time_steps(fn, steps, warmup)
        byts = BYTES_PER_ELEMENT[name] * n
        floor = byts / HBM_ACHIEVABLE * 1e3
        res["legs"][name] = dict(median_ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4), bytes_per_step=byts,
                                 achieved_tb_s=round(byts / (med * 1e-3) / 1e12, 3), floor_ms_at_6p3_tb_s=round(floor, 4),
                                 floor_ms_at_8_tb_s=round(byts / HBM_SPEC * 1e3, 4), time_over_floor=round(med / floor, 3))
        if name == "fused":
            del opt
        torch.cuda.synchronize()
    if "loop" in res["legs"] and "fused" in res["legs"]:
        res["loop_over_fused"] = round(res["legs"]["loop"]["median_ms"] / res["legs"]["fused"]["median_ms"], 2)
    return res


def merge_kernel_stats(path, db_path, steps_per_size=23, sizes=("base", "large")):
    """Median per-kernel times of the fused step from a rocprofv3 (rocpd SQLite) kernel trace of `--only fused` runs over
    `sizes`, steps_per_size launches of each kernel per size, merged into the JSON at path."""
    import sqlite3
    with open(path) as f:
        out = json.load(f)
    rows = sqlite3.connect(db_path).execute("select name, start, end from kernels order by start").fetchall()
    ks = {}
    for name, s, e in rows:
        for k in ("lamb_pass1_kernel", "lamb_reduce_kernel", "lamb_pass2_kernel"):
            if k in name:
                ks.setdefault(k, []).append((e - s) / 1e3)
    stats = {}
    for i, size in enumerate(sizes):
        d = {k: round(statistics.median(v[i * steps_per_size:(i + 1) * steps_per_size]), 2) for k, v in ks.items()}
        n = out[size]["n_elements_with_grad"]
        d["sum_us"] = round(sum(d.values()), 2)
        d["pass1_tb_s"] = round(24 * n / (d["lamb_pass1_kernel"] * 1e-6) / 1e12, 3)
        d["pass2_tb_s"] = round(16 * n / (d["lamb_pass2_kernel"] * 1e-6) / 1e12, 3)
        d["kernels_over_floor"] = round(d["sum_us"] * 1e-3 / out[size]["legs"]["fused"]["floor_ms_at_6p3_tb_s"], 3)
        stats[size] = d
    out["rocprofv3_kernel_trace"] = dict(note="separate run (rocprofv3 --kernel-trace), fused leg only, %d launches per size "
                                         "(warm-up included); median kernel time in us" % steps_per_size, **stats)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(stats, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="base,large")
    ap.add_argument("--only", default="all", choices=["all", "fused"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_lamb_step.json"))
    ap.add_argument("--kernel-stats", default=None, help="merge the kernel times of a rocprofv3 results .db into --out and exit")
    a = ap.parse_args()
    if a.kernel_stats:
        merge_kernel_stats(a.out, a.kernel_stats)
        return
    import torch
    assert torch.cuda.is_available(), "bench_lamb.py times the GPU; there is no CPU measurement"
    out = dict(what="one LAMB optimizer step, RobertaDot_NLL_LN parameters, run_ann.py grouping", device=torch.cuda.get_device_name(0),
               torch=torch.__version__, steps=a.steps, warmup=a.warmup, hbm_floor_basis="6.3 TB/s achievable (8 TB/s spec alongside)")
    for kind in a.sizes.split(","):
        out[kind] = bench(kind, a.steps, a.warmup, a.only)
        print(kind, json.dumps(out[kind]), flush=True)
        torch.cuda.empty_cache()
    if a.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
