"""Times the tail of a trainer's step -- everything that is not the towers -- with device events, medians, one process, the
variants alternated --rounds times (each round times every variant once, --steps steps after --warmup):

 1. optimizer tail on RobertaDot_NLL_LN's parameters (RoBERTa-base and -large shapes, tests/lamb_util.py, run_ann.py's grouping)
    (a) clipped   ance_amd.optim.Lamb(max_grad_norm=1.0).step()            -> ance_lamb_step_clipped, 44 B per element
    (b) unfused   torch.nn.utils.clip_grad_norm_(params, 1.0); Lamb.step()  -> 52 B per element and a dozen launches more
    (c) plain     Lamb.step() alone                                        -> 40 B per element (profiles/r07_lamb_step.json's leg)
    (d) the 44 B per element HBM floor at the copy rate scripts/bench_lamb.py uses
    under loss scaling (RoBERTa-base shapes; torch.amp.GradScaler at 2^16, Lamb(max_grad_norm=1.0)):
    (e) amp_fused    scaler.step(opt); scaler.update()  -> ance_lamb_step_amp unscales in registers and skips on the device
    (f) amp_unfused  what a Lamb without _step_supports_amp_scaling does: scaler.unscale_(opt), the clipped step behind the
                     scaler's found_inf .item(), update()
    Both keep the scaler's own finite-check pass over the gradients, so by bytes (e) is no lighter than (f) minus the 8 B per
    element of unscale_'s rewrite; what (e) removes is the host wait and launches.  Launch counts: a separate
    `rocprofv3 --kernel-trace --stats` run of `--trace amp:amp_fused` / `--trace amp:amp_unfused` (--trace-calls steps and nothing
    else; the parameters' upload adds a fixed number of kernels, which the difference of two call counts removes).
 2. objective forward + backward at the trainers' sizes against the reference's torch expression on the same tensors: triplets
    n = 8, 32, 128 (FirstP; MaxP 4 chunks), in-batch 128 x 256 and 1024 x 2048.  Launch-bound: the figure of merit is the launch
    count (from a separate `rocprofv3 --kernel-trace --stats` run of `--trace CASE:VARIANT`, which makes --trace-calls calls and
    nothing else; the inputs' random fill adds a fixed handful of kernels, which the difference of two call counts removes) and
    the absence of host waits.

Writes one JSON object (--out, default profiles/r08_step_tail.json)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_ACHIEVABLE = 6.3e12  # B/s: MI355X float4 copy, as scripts/bench_lamb.py
BYTES = {"clipped": 44, "unfused": 52, "plain": 40}


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


def alternate(legs, rounds, steps, warmup):
    """{name: dict(median_ms of the rounds' medians, rounds_ms, spread_ms = max - min over the rounds)}"""
    seen = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            seen[name].append(time_steps(fn, steps, warmup))
    return {name: dict(median_ms=round(statistics.median(v), 4), rounds_ms=[round(x, 4) for x in v], spread_ms=round(max(v) - min(v), 4))
            for name, v in seen.items()}


def bench_optimizer(kind, rounds, steps, warmup):
    import torch
    import lamb_util as U
    from ance_amd.optim import Lamb
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)

    def build():
        groups, n = [], 0
        for gname, plist in U.roberta_param_groups(kind):
            ps = []
            for name, t, has_grad in plist:
                p = torch.nn.Parameter(t.to(dev))
                if has_grad:
                    p.grad = torch.randn(t.shape, device=dev, generator=gen) * 1e-3
                    n += p.numel()
                ps.append(p)
            groups.append(dict(params=ps))
        return groups, n

    # one parameter set per variant: the variants must not step each other's state
    sets = {name: build() for name in ("clipped", "unfused", "plain")}
    n = sets["plain"][1]
    opt = {"clipped": Lamb(sets["clipped"][0], lr=1e-4, eps=1e-6, max_grad_norm=1.0),
           "unfused": Lamb(sets["unfused"][0], lr=1e-4, eps=1e-6), "plain": Lamb(sets["plain"][0], lr=1e-4, eps=1e-6)}
    unfused_params = [p for g in sets["unfused"][0] for p in g["params"]]

    def unfused():
        # clip_grad_norm_ rescales p.grad in memory, so from the second call on the norm is at most 1: torch still reads every
        # gradient for the norm and multiplies every gradient by the clamped factor (1), which is a training step's traffic
        torch.nn.utils.clip_grad_norm_(unfused_params, 1.0)
        opt["unfused"].step()

    legs = {"clipped": opt["clipped"].step, "unfused": unfused, "plain": opt["plain"].step}
    res = dict(n_elements_with_grad=n, legs=alternate(legs, rounds, steps, warmup))
    for name, leg in res["legs"].items():
        byts = BYTES[name] * n
        leg.update(bytes_per_step=byts, achieved_tb_s=round(byts / (leg["median_ms"] * 1e-3) / 1e12, 3),
                   floor_ms_at_6p3_tb_s=round(byts / HBM_ACHIEVABLE * 1e3, 4))
    spread = max(leg["spread_ms"] for leg in res["legs"].values())
    res["floor_44B_ms_at_6p3_tb_s"] = round(44 * n / HBM_ACHIEVABLE * 1e3, 4)
    res["unfused_minus_clipped_ms"] = round(res["legs"]["unfused"]["median_ms"] - res["legs"]["clipped"]["median_ms"], 4)
    res["largest_spread_of_the_alternations_ms"] = spread
    res["clipped_faster_than_unfused_by_more_than_the_spread"] = res["unfused_minus_clipped_ms"] > spread
    return res


def amp_legs(kind="base"):
    """{amp_fused, amp_unfused}: one GradScaler step each on a parameter set of its own (gradients stay in memory: unscale_ shrinks
    them call after call towards zero, which changes no traffic), and the number of elements with a gradient."""
    import torch
    import lamb_util as U
    from ance_amd.optim import Lamb
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(2)

    class UnfusedLamb(Lamb):  # the optimizer as it was before it spoke the scaler's contract: GradScaler takes its unfused branch
        _step_supports_amp_scaling = False

    legs, n = {}, 0
    for name, cls in (("amp_fused", Lamb), ("amp_unfused", UnfusedLamb)):
        groups, n = [], 0
        for gname, plist in U.roberta_param_groups(kind):
            ps = []
            for pname, t, has_grad in plist:
                p = torch.nn.Parameter(t.to(dev))
                if has_grad:
                    p.grad = torch.randn(t.shape, device=dev, generator=gen) * 1e-3
                    n += p.numel()
                ps.append(p)
            groups.append(dict(params=ps))
        opt = cls(groups, lr=1e-4, eps=1e-6, max_grad_norm=1.0)
        scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16, growth_interval=1 << 30)
        scaler.scale(torch.zeros((), device=dev))

        def fused(opt=opt, scaler=scaler):
            scaler.step(opt)
            scaler.update()

        def unfused(opt=opt, scaler=scaler):
            scaler.unscale_(opt)
            scaler.step(opt)
            scaler.update()

        legs[name] = fused if cls is Lamb else unfused
    return legs, n


def bench_amp(rounds, steps, warmup):
    legs, n = amp_legs("base")
    res = dict(n_elements_with_grad=n, scale=65536.0, max_grad_norm=1.0, legs=alternate(legs, rounds, steps, warmup))
    res["amp_unfused_minus_amp_fused_ms"] = round(res["legs"]["amp_unfused"]["median_ms"] - res["legs"]["amp_fused"]["median_ms"], 4)
    res["largest_spread_of_the_alternations_ms"] = max(leg["spread_ms"] for leg in res["legs"].values())
    return res


def objective_cases():
    import torch
    import torch.nn.functional as F
    from ance_amd.loss import biencoder_nll_loss, nll_loss
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)

    def rnd(*shape, std=0.05):
        return (torch.randn(shape, device=dev, generator=gen) * std).requires_grad_(True)

    cases = {}
    for n in (8, 32, 128):
        for chunks in (1, 4):
            q = rnd(n, 768)
            a, b = (rnd(n, 768, std=1.0), rnd(n, 768, std=1.0)) if chunks == 1 else (rnd(n, chunks, 768, std=1.0), rnd(n, chunks, 768, std=1.0))
            ma = mb = None
            if chunks > 1:
                ma = (torch.arange(chunks, device=dev)[None, :] < (1 + torch.arange(n, device=dev) % chunks)[:, None]).float()
                mb = ma.flip(0).contiguous()

            def ours(q=q, a=a, b=b, ma=ma, mb=mb):
                q.grad = a.grad = b.grad = None
                nll_loss(q, a, b, ma, mb).backward()

            def ref(q=q, a=a, b=b, ma=ma, mb=mb, chunks=chunks):
                q.grad = a.grad = b.grad = None
                if chunks == 1:
                    la, lb = (q * a).sum(-1), (q * b).sum(-1)
                else:
                    la = (torch.matmul(q.unsqueeze(1), a.transpose(1, 2))[:, 0, :] + (1 - ma) * -9999).max(dim=-1).values
                    lb = (torch.matmul(q.unsqueeze(1), b.transpose(1, 2))[:, 0, :] + (1 - mb) * -9999).max(dim=-1).values
                lsm = F.log_softmax(torch.cat([la.unsqueeze(1), lb.unsqueeze(1)], dim=1), dim=1)
                (-1.0 * lsm[:, 0]).mean().backward()

            cases["triplet_n%d_chunks%d" % (n, chunks)] = (ours, ref)
    for nq, nc in ((128, 256), (1024, 2048)):
        q, c = rnd(nq, 768), rnd(nc, 768)
        pos = torch.arange(nq, device=dev) * 2

        def ours(q=q, c=c, pos=pos):
            q.grad = c.grad = None
            biencoder_nll_loss(q, c, pos)[0].backward()

        def ref(q=q, c=c, pos=pos):
            q.grad = c.grad = None
            lsm = F.log_softmax(torch.matmul(q, c.t()), dim=1)
            loss = F.nll_loss(lsm, pos, reduction="mean")
            (torch.max(lsm, 1)[1] == pos).sum()
            loss.backward()

        cases["inbatch_%dx%d" % (nq, nc)] = (ours, ref)
    return cases


def bench_objectives(rounds, steps, warmup):
    out = {}
    for name, (ours, ref) in objective_cases().items():
        r = alternate({"ance_amd": ours, "torch_expression": ref}, rounds, steps, warmup)
        out[name] = dict(ance_amd_ms=r["ance_amd"]["median_ms"], torch_expression_ms=r["torch_expression"]["median_ms"],
                         ance_amd_rounds_ms=r["ance_amd"]["rounds_ms"], torch_expression_rounds_ms=r["torch_expression"]["rounds_ms"])
        print(name, json.dumps(out[name]), flush=True)
    return out


def trace_calls(spec, calls):
    """For a `rocprofv3 --kernel-trace --stats` run of its own: CASE:VARIANT called `calls` times and nothing else on the GPU, so
    the launches per call are the trace's kernel count divided by `calls`."""
    import torch
    case, variant = spec.split(":")
    fn = amp_legs()[0][variant] if case == "amp" else objective_cases()[case][0 if variant == "ance_amd" else 1]
    torch.cuda.synchronize()
    print("TRACE_BEGIN %s calls=%d" % (spec, calls), flush=True)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the variants (at least three)")
    ap.add_argument("--sizes", default="base,large")
    ap.add_argument("--skip-objectives", action="store_true")
    ap.add_argument("--trace", default=None, help="CASE:VARIANT (VARIANT ance_amd or torch_expression; amp:amp_fused or amp:amp_unfused): "
                    "only call it, for a kernel trace")
    ap.add_argument("--skip-amp", action="store_true")
    ap.add_argument("--amp-launches", default=None, help="FUSED,UNFUSED: traced kernel launches per GradScaler step, recorded in the output")
    ap.add_argument("--trace-calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_step_tail.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_step_tail.py times the GPU; there is no CPU measurement"
    if a.trace:
        trace_calls(a.trace, a.trace_calls)
        return
    assert a.rounds >= 3
    out = dict(what="the tail of a trainer's step: clip + LAMB (also under a GradScaler), and the objectives' forward + backward",
               device=torch.cuda.get_device_name(0), torch=torch.__version__, steps=a.steps, warmup=a.warmup, rounds=a.rounds,
               hbm_floor_basis="6.3 TB/s achievable copy rate", optimizer={})
    for kind in [k for k in a.sizes.split(",") if k]:
        out["optimizer"][kind] = bench_optimizer(kind, a.rounds, a.steps, a.warmup)
        print(kind, json.dumps(out["optimizer"][kind]), flush=True)
        torch.cuda.empty_cache()
    if not a.skip_amp:
        out["amp"] = bench_amp(a.rounds, a.steps, a.warmup)
        if a.amp_launches:
            fused, unfused = (float(x) for x in a.amp_launches.split(","))
            out["amp"]["traced_launches_per_step"] = dict(amp_fused=fused, amp_unfused=unfused)
        print("amp", json.dumps(out["amp"]), flush=True)
        torch.cuda.empty_cache()
    if not a.skip_objectives:
        out["objectives"] = bench_objectives(a.rounds, a.steps, a.warmup)
    if a.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
