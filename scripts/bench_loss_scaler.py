"""Times the loss scaler -- ance_amd.optim.LossScaler, whose overflow check is part of the fused optimizer step, against
torch.amp.GradScaler, whose step() walks the parameters and reads every gradient once more -- in ONE process, the variants
alternated --rounds times and every round kept.

  optimizer tail alone   RoBERTa-base's 201 gradient tensors (tests/lamb_util.py's roberta_param_groups), Lamb and AdamW with
                         max_grad_norm=1.0: GradScaler.step + update (the flow before this feature) against LossScaler.step + update.
                         Host enqueue ms, device-event ms, and the launches and copies of one traced tail.
  the whole step         scripts/bench_graph_step.py's 12-layer triplet step under torch.autocast(fp16) with precision="half", at both
                         shapes: eager in device mode and replayed from one captured graph, with a LossScaler, with a GradScaler where
                         torch's scaler captures (its error text otherwise), and without any scaler (the replay that was measured
                         before).

No speed-up is asserted anywhere: the JSON holds what was measured."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_graph_step import CFG, SHAPES, TOTAL, WARM, batches, rounds_of, traced, window  # noqa: E402


def make_scaler(which):
    import torch
    from ance_amd.optim import LossScaler
    if which == "loss_scaler":
        return LossScaler(init_scale=65536.0, growth_interval=2000)
    if which == "grad_scaler":
        return torch.amp.GradScaler("cuda", init_scale=65536.0, growth_interval=2000)
    return None


def bench_tail(rounds, steps, warmup):
    """scaler.step(optimizer) + scaler.update() on gradients that are already there (scaled by 65536, all finite)."""
    import torch
    import lamb_util as U
    from ance_amd.optim import AdamW, Lamb
    dev = torch.device("cuda:0")
    host = U.roberta_param_groups("base")
    res = {}
    for kind, Opt in (("lamb_clip", Lamb), ("adamw_clip", AdamW)):
        legs = {}
        for which in ("grad_scaler", "loss_scaler"):
            gen = torch.Generator(device=dev).manual_seed(0)
            groups = []
            for _, plist in host:
                ps = []
                for _, t, has_grad in plist:
                    p = torch.nn.Parameter(t.to(dev))
                    if has_grad:
                        p.grad = torch.randn(t.shape, device=dev, generator=gen) * (1e-3 * 65536.0)
                    ps.append(p)
                groups.append(dict(params=ps))
            opt = Opt(groups, lr=1e-4, eps=1e-6, weight_decay=0.01, max_grad_norm=1.0)
            scaler = make_scaler(which)
            scaler.scale(torch.zeros((), device=dev))   # the scaler's device state

            def tail(opt=opt, scaler=scaler):
                scaler.step(opt)
                scaler.update()

            legs[which] = (tail, opt)
        seen = {name: [] for name in legs}
        for _ in range(rounds):
            for name, (fn, _) in legs.items():
                for _ in range(warmup):
                    fn()
                seen[name].append(window(fn, steps))
        out = {}
        for name, (fn, opt) in legs.items():
            v = seen[name]
            out[name] = dict(host_enqueue_ms_per_step=rounds_of(v, 0), device_event_ms_per_step=rounds_of(v, 2), traced_tail=traced(fn),
                             skipped_steps=int(opt.skipped_steps.item()))
        res[kind] = out
        del legs
        torch.cuda.empty_cache()
    return res


def make_step(which, replay, sd, B, lens3):
    """One step of the fp16 tower with scaler `which` (None: no scaler), eager in device mode or replayed from one graph.  Returns the
    closure, or the text of the error the capture raised."""
    import torch
    import lamb_util as U
    import train_step_util as S
    from ance_amd import attention as T
    from ance_amd.loss import nll_loss
    from ance_amd.optim import Lamb, LinearWarmupSchedule
    tower = S.device_tower(CFG, sd, 0.1, precision="half").train()
    opt = Lamb(S.param_groups(tower), lr=1e-3, betas=U.BETAS, eps=U.EPS, max_grad_norm=1.0)
    gen = torch.Generator(device="cuda:0").manual_seed(5)
    static = batches(B, lens3, S.VOCAB, gen)
    sched = LinearWarmupSchedule(opt, WARM, TOTAL)
    scaler = make_scaler(which)

    def step():
        with torch.autocast("cuda", dtype=torch.float16):
            loss = nll_loss(*[tower(*c) for c in static])
        if scaler is None:
            loss.backward()
            opt.step()
        else:
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
        sched.step()
        T.dropout_state.advance(0)

    def eager():
        step()
        opt.zero_grad(set_to_none=True)

    if not replay:
        return eager
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            eager()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph):
            step()
    except Exception as e:   # torch's scaler may refuse the capture: the text is the result
        torch.cuda.synchronize()
        return "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:300])
    return graph.replay


def bench_steps(rounds, steps, warmup):
    import torch
    import train_step_util as S
    from ance_amd import attention as T
    sd = S.tower_state(CFG)
    T.dropout_state.to_device(0)
    res = {}
    for shape, (B, lens3) in SHAPES.items():
        legs, errors = {}, {}
        for which in ("no_scaler", "loss_scaler", "grad_scaler"):
            for replay in (False, True):
                if which == "no_scaler" and not replay:
                    continue
                name = "%s %s" % (which, "graph_replay" if replay else "eager_device")
                made = make_step(None if which == "no_scaler" else which, replay, sd, B, lens3)
                if isinstance(made, str):
                    errors[name] = made
                else:
                    legs[name] = made
        seen = {name: [] for name in legs}
        for _ in range(rounds):
            for name, fn in legs.items():
                for _ in range(warmup):
                    fn()
                seen[name].append(window(fn, steps))
            print(shape, "round", {k: [round(x, 3) for x in v[-1]] for k, v in seen.items()}, flush=True)
        out = {}
        for name, fn in legs.items():
            v = seen[name]
            out[name] = dict(host_enqueue_ms_per_step=rounds_of(v, 0), wall_ms_per_step=rounds_of(v, 1),
                             device_event_ms_per_step=rounds_of(v, 2), traced_step=traced(fn))
        for name, text in errors.items():
            out[name] = dict(capture_error=text)
        res["autocast_fp16_half " + shape] = out
        del legs
        torch.cuda.empty_cache()
    T.dropout_state.to_host(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_loss_scaler.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_loss_scaler.py times the GPU; there is no CPU measurement"
    assert a.rounds >= 5, "at least five rounds, every round kept"
    out = dict(what="the loss scaler: the optimizer tail alone (scaler.step + scaler.update over RoBERTa-base's 201 gradient tensors) under "
                    "torch.amp.GradScaler and under ance_amd.optim.LossScaler, and the whole 12-layer fp16 triplet step eager and replayed "
                    "from one captured graph with either scaler and with none",
               device=torch.cuda.get_device_name(0), torch=torch.__version__, rounds=a.rounds, steps_per_window=a.steps, warmup=a.warmup,
               note="one process, variants alternated, every round kept; a replayed graph is traced as one graph launch (0 kernels)")
    out["optimizer_tail_roberta_base"] = bench_tail(a.rounds, 20, 3)
    out["whole_step"] = bench_steps(a.rounds, a.steps, a.warmup)
    print(json.dumps(out), flush=True)
    if a.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
