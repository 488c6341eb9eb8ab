"""Times the input end of a trainable tower -- ids -> word + token_type + position -> LayerNorm -> dropout, forward + backward with
dense table gradients -- with device events, in ONE process, the variants alternated --rounds times (each round times every variant
once: --steps steps after --warmup):
  eager   the installed transformers' RobertaEmbeddings / BertEmbeddings modules (what a trainer assembled from this package falls
          back on without ance_amd.embeddings)
  fused   ance_amd.embeddings.BertEmbeddings -> csrc/embed_train.hip (one launch forward; four of its own backward, plus torch's
          stable sorts that group the rows by id)
A step is the three tower calls of a training step one after another (query batch, positive batch, negative batch: each its own
padded [B, L] with its own lengths), each forward + backward, in training mode with dropout 0.1, fp32, real vocabulary sizes; the
parameter gradients are dropped between steps.  Shapes and seeded lengths are scripts/bench_attention_train.py's:
  warmup   32 x (64, 128, 128)     RoBERTa tower (vocab 50265, 514 positions, roberta position ids)
  firstp   8 x (64, 512, 512)      RoBERTa tower
  maxp     2 x (64 + 2 x 8 chunks of 512)   RoBERTa tower
  dpr      16 x (256, 256, 256)    BERT tower (vocab 30522, 512 positions, two token types)
Per variant and shape: device-event time of a step (median and best of the rounds' window medians, every round kept), host enqueue
time of a step (perf_counter around the calls, no synchronise inside), torch.cuda.max_memory_allocated over a step above what was
allocated before it, and the launches of one step traced with torch.profiler (after the timing).  No ratio is a criterion: the step
time of a tower is elsewhere.  Writes one JSON object (--out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

H, P_DROP = 768, 0.1
TOWERS = {"roberta": dict(vocab=50265, max_pos=514, n_types=1, pad=1, eps=1e-5, mode="roberta"),
          "bert": dict(vocab=30522, max_pos=512, n_types=2, pad=0, eps=1e-12, mode="absolute")}
TOWER_OF = {"warmup": "roberta", "firstp": "roberta", "maxp": "roberta", "dpr": "bert"}


def build(tower):
    """(eager module, fused module) on the device with the same parameter values."""
    import torch
    from transformers import BertConfig, RobertaConfig
    from transformers.models.bert.modeling_bert import BertEmbeddings as HFBert
    from transformers.models.roberta.modeling_roberta import RobertaEmbeddings as HFRoberta
    from ance_amd.embeddings import BertEmbeddings
    t = TOWERS[tower]
    kw = dict(vocab_size=t["vocab"], hidden_size=H, max_position_embeddings=t["max_pos"], type_vocab_size=t["n_types"],
              layer_norm_eps=t["eps"], hidden_dropout_prob=P_DROP, pad_token_id=t["pad"])
    torch.manual_seed(0)
    eager = (HFRoberta(RobertaConfig(**kw)) if tower == "roberta" else HFBert(BertConfig(**kw))).to("cuda:0").train()
    fused = BertEmbeddings(t["vocab"], H, t["max_pos"], t["n_types"], t["eps"], P_DROP, pad_token_id=t["pad"], position_mode=t["mode"]).to("cuda:0").train()
    fused.load_state_dict(eager.state_dict(), strict=True)
    return eager, fused


def step_inputs(calls, tower, seed=0):
    """Per tower call: ids [B, L] int64 (pad beyond each length) and the gradient arriving at the output."""
    import numpy as np
    import torch
    t = TOWERS[tower]
    rng = np.random.default_rng(seed)
    gen = torch.Generator(device="cuda:0").manual_seed(seed)
    out = []
    for L, lens in calls:
        ids = rng.integers(t["pad"] + 2, t["vocab"], size=(len(lens), L))
        ids = np.where(np.arange(L)[None, :] < np.asarray(lens)[:, None], ids, t["pad"])
        out.append((torch.from_numpy(ids).to("cuda:0"), torch.randn(len(lens), L, H, device="cuda:0", generator=gen)))
    return out


def make_step(module, inputs, eager):
    def step():
        for ids, dy in inputs:
            y = module(input_ids=ids) if eager else module(ids)
            y.backward(dy)
        module.zero_grad(set_to_none=True)
    return step


def time_steps(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    host = []
    for a, b in ev:
        a.record()
        t0 = time.perf_counter()
        fn()
        host.append((time.perf_counter() - t0) * 1e3)
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev), statistics.median(host)


def peak_bytes(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def traced(fn):
    """Kernel launches, copies / memsets and the summed device time of one step, from torch.profiler."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    kernels = copies = ours = 0
    device_us = 0.0
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            if "memcpy" in e.name.lower() or "memset" in e.name.lower():
                copies += 1
            else:
                kernels += 1
                ours += "ance::" in e.name
            device_us += float(getattr(e, "device_time", getattr(e, "cuda_time", 0.0)))
    return dict(kernels=kernels, of_which_this_library=ours, copies_and_memsets=copies, device_time_us=round(device_us, 1))


def bench(name, calls, rounds, steps, warmup, trace):
    import torch
    tower = TOWER_OF[name]
    eager, fused = build(tower)
    inputs = step_inputs(calls, tower)
    variants = {"eager": make_step(eager, inputs, True), "fused": make_step(fused, inputs, False)}
    seen = {v: dict(event=[], host=[]) for v in variants}
    for _ in range(rounds):
        for vname, fn in variants.items():
            ev, host = time_steps(fn, steps, warmup)
            seen[vname]["event"].append(ev)
            seen[vname]["host"].append(host)
        print(name, "round", {k: round(v["event"][-1], 4) for k, v in seen.items()}, flush=True)
    out = {}
    for vname, fn in variants.items():
        ev, host = seen[vname]["event"], seen[vname]["host"]
        out[vname] = dict(step_event_ms=dict(median=round(statistics.median(ev), 4), best=round(min(ev), 4), rounds=[round(x, 4) for x in ev]),
                          step_host_enqueue_ms=dict(median=round(statistics.median(host), 4), best=round(min(host), 4),
                                                    rounds=[round(x, 4) for x in host]),
                          peak_bytes_over_a_step=peak_bytes(fn))
        if trace:
            try:
                out[vname]["traced_step"] = traced(fn)
            except Exception as e:  # pragma: no cover - depends on the profiler of the torch build
                out[vname]["traced_step"] = dict(unavailable=repr(e))
    e, f = out["eager"]["step_event_ms"], out["fused"]["step_event_ms"]
    spread = max(max(e["rounds"]) - min(e["rounds"]), max(f["rounds"]) - min(f["rounds"]))
    res = dict(tower=tower, calls=[dict(L=int(L), B=int(len(lens)), tokens=int(sum(lens))) for L, lens in calls], variants=out,
               eager_over_fused_step_event=round(e["median"] / f["median"], 3),
               fused_faster_than_eager_by_more_than_the_spread=bool(e["median"] - f["median"] > spread),
               fused_peak_memory_lower_than_eager=bool(out["fused"]["peak_bytes_over_a_step"] < out["eager"]["peak_bytes_over_a_step"]))
    del eager, fused, variants
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="warmup,firstp,maxp,dpr")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_embeddings.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_embeddings.py times the GPU; there is no CPU measurement"
    import transformers
    from ance_amd import attention
    from bench_attention_train import shapes
    attention.manual_seed(0)
    all_shapes = shapes()
    out = dict(what="BertEmbeddings / RobertaEmbeddings forward + backward of the three tower calls of a step, fp32, training mode, dropout 0.1, "
                    "hidden 768, real vocabulary sizes; the installed transformers' eager modules against ance_amd.embeddings.BertEmbeddings",
               device=torch.cuda.get_device_name(0), torch=torch.__version__, transformers=transformers.__version__,
               timing=dict(rounds=a.rounds, steps_per_window=a.steps, warmup_steps=a.warmup))
    for name in a.shapes.split(","):
        out[name] = bench(name, all_shapes[name], a.rounds, a.steps, a.warmup, not a.no_trace)
        print(name, json.dumps(out[name]), flush=True)
    if a.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
