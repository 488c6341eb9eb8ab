"""Times a WHOLE training step of RobertaDot_NLL_LN (ance_amd/model.py: the last layer computes its first rows only) against the
composition a trainer had before it -- stated here as ParentModel: the same BertEmbeddings and BertLayers, the FULL last layer, then
h[:, 0] into torch's nn.Linear(H, 768) + nn.LayerNorm(768) -- in ONE process, the variants alternated --rounds times, every round kept.
12 layers at RoBERTa-base width, seeded weights (both variants load the same), dropout 0.1, three tower calls + the triplet objective
+ backward + Lamb(max_grad_norm=1.0), at the shapes of scripts/bench_graph_step.py: B x (Lq, Ld, Ld) = 8 x (64, 512, 512) and
32 x (64, 128, 128); fp32, and torch.autocast(fp16) with precision="half" (no GradScaler); eager (device dropout stream) and replayed
from one captured graph.  Per leg: wall ms per step, the kernel launches and copies of one traced step, peak memory of a step.
By FLOP count from shapes the last layer sheds 10 of its 12 H^2-sized GEMM units (about 7 % of the layers' matrix work at N = 12):
an estimate; the JSON holds what was measured and no speed-up is asserted.

The kernel trace is a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -o row0 -- python scripts/bench_tower.py --trace-call
    python scripts/bench_tower.py --fold-stats DIR/.../row0_kernel_stats.csv
--trace-call runs attention_first_row and attention_padded (dctx nonzero in row 0 only), forward + backward, TRACE_REPS times on one
call; --fold-stats adds the row-0 kernels' and the full core's device time to the JSON, with the bytes computed here from the shapes
(forward: K and V read; backward: K and V read, dK and dV written) as a share of the HBM peak."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"8x(64,512,512)": (8, (64, 512, 512)), "32x(64,128,128)": (32, (64, 128, 128))}
CFG = dict(H=768, heads=12, inter=3072, N=12, mode="roberta", n_types=1, eps=1e-5, pad=1)
TRACE_SHAPE, TRACE_REPS = (32, 512, 12), 20   # B, L, heads of the traced call
HBM_PEAK_BYTES_PER_S = 8.0e12                 # MI355X: 8 TB/s


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
    """wall ms per step of a window of steps with one synchronise behind it."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def parent_model(config, precision):
    """The parent's composition: every layer full, the head torch's own modules."""
    import torch
    from ance_amd.attention import lens_from_mask
    from ance_amd.model import _Tower

    class ParentModel(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.roberta = _Tower(config, "roberta", precision)   # the same modules and names; its forward is not used
            self.embeddingHead = torch.nn.Linear(config.hidden_size, 768)
            self.norm = torch.nn.LayerNorm(768)

        def emb(self, ids, mask):
            lens = lens_from_mask(mask)
            h = self.roberta.embeddings(ids)
            layers = self.roberta.encoder.layer
            if precision == "half":
                h16 = None
                for layer in layers[:-1]:
                    h, h16 = layer(h, lens, hidden_states_half=h16, return_half=True)
                h = layers[-1](h, lens, hidden_states_half=h16)
            else:
                for layer in layers:
                    h = layer(h, lens)
            return self.norm(self.embeddingHead(h[:, 0].contiguous())).float()

    return ParentModel()


def batches(B, lens3, vocab, gen):
    import torch
    out = []
    for L in lens3:
        ids = torch.randint(2, vocab, (B, L), device="cuda:0", generator=gen)
        lens = torch.randint(max(1, L // 2), L + 1, (B,), device="cuda:0", generator=gen)
        mask = (torch.arange(L, device="cuda:0")[None, :] < lens[:, None]).long()
        out += [ids * mask + (1 - mask), mask]
    return out


def make_leg(variant, graph, sd, B, lens3, half):
    import torch
    import lamb_util as U
    import train_step_util as S
    from ance_amd import attention as T
    from ance_amd import model
    from ance_amd.loss import nll_loss
    from ance_amd.optim import Lamb
    precision = "half" if half else "fp32"
    config = model.TowerConfig(S.VOCAB, CFG["H"], CFG["N"], CFG["inter"], S.MAX_POS, 1, CFG["eps"], CFG["pad"], 0.1, 0.1)
    if variant == "model":
        m = model.RobertaDot_NLL_LN(config, precision=precision)
        emb = m.query_emb
    else:
        m = parent_model(config, precision)
        emb = m.emb
    m = m.to("cuda:0").train()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    named = list(m.named_parameters())
    groups = [dict(params=[q for n, q in named if S.group_of(n.replace("roberta.", "")) == k], lr=U.GROUPS[k]["lr"],
                   weight_decay=U.GROUPS[k]["weight_decay"]) for k in range(len(U.GROUPS))]
    opt = Lamb(groups, lr=1e-3, betas=U.BETAS, eps=U.EPS, max_grad_norm=1.0)
    static = batches(B, lens3, S.VOCAB, torch.Generator(device="cuda:0").manual_seed(5))

    def step():
        with torch.autocast("cuda", dtype=torch.float16, enabled=half):
            loss = nll_loss(emb(static[0], static[1]), emb(static[2], static[3]), emb(static[4], static[5]))
        loss.backward()
        opt.step()
        T.dropout_state.advance(0)

    def eager():
        step()
        opt.zero_grad(set_to_none=True)

    T.dropout_state.to_device(0)
    if not graph:
        return eager
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            eager()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    return g.replay


def peak_memory(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated())


def bench(rounds, steps, warmup):
    import torch
    import model_util as M
    sd = M.model_state(CFG)
    res = {}
    for half in (False, True):
        for shape, (B, lens3) in SHAPES.items():
            key = "%s %s" % ("autocast_fp16_half" if half else "fp32", shape)
            legs = {"%s_%s" % (v, "graph" if g else "eager"): make_leg(v, g, sd, B, lens3, half)
                    for g in (False, True) for v in ("parent", "model")}
            seen = {name: [] for name in legs}
            for _ in range(rounds):
                for name, fn in legs.items():
                    for _ in range(warmup):
                        fn()
                    seen[name].append(window(fn, steps))
                print(key, "round", {k: round(v[-1], 3) for k, v in seen.items()}, flush=True)
            out = {}
            for name, fn in legs.items():
                v = seen[name]
                out[name] = dict(wall_ms_per_step=dict(median=round(statistics.median(v), 4), rounds=[round(x, 4) for x in v]),
                                 traced_step=traced(fn), peak_bytes_of_a_step=peak_memory(fn))
            for mode in ("eager", "graph"):
                a, b = out["parent_" + mode]["wall_ms_per_step"], out["model_" + mode]["wall_ms_per_step"]
                out["model_over_parent_" + mode] = dict(ratio_of_medians=round(b["median"] / a["median"], 4),
                                                        parent_spread_ms=round(max(a["rounds"]) - min(a["rounds"]), 4),
                                                        model_spread_ms=round(max(b["rounds"]) - min(b["rounds"]), 4))
            res[key] = out
            del legs
            torch.cuda.empty_cache()
    return res


def trace_call():
    """The traced call: both cores, forward + backward, on one set of inputs."""
    import torch
    from ance_amd.attention import attention_first_row, attention_padded
    B, L, nh = TRACE_SHAPE
    H = 64 * nh
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    q, k, v = (torch.randn(B, L, H, device="cuda:0", generator=gen).requires_grad_(True) for _ in range(3))
    lens = torch.full((B,), L, device="cuda:0", dtype=torch.int32)
    g0 = torch.randn(B, H, device="cuda:0", generator=gen)
    g = torch.zeros(B, L, H, device="cuda:0")
    g[:, 0] = g0
    q0 = q.detach()[:, 0].clone().requires_grad_(True)
    for _ in range(TRACE_REPS):
        attention_first_row(q0, k, v, lens, nh, 0.1, True).backward(g0)
        attention_padded(q, k, v, lens, nh, 0.1, True).backward(g)
    torch.cuda.synchronize()


def fold_stats(path, out_path):
    B, L, nh = TRACE_SHAPE
    kv = 2 * B * L * 64 * nh * 4   # K and V (or dK and dV), fp32
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            rows[r["Name"]] = (int(r["Calls"]), float(r["TotalDurationNs"]))
    kernels = {}
    for name, (calls, total) in rows.items():
        if "row0_" in name or "attn_" in name or "attention" in name.lower():
            kernels[name] = dict(calls=calls, mean_us=round(total / calls / 1e3, 3))
    summary = {}
    for tag, nbytes in (("row0_fwd", kv), ("row0_bwd", 2 * kv)):
        hit = [(n, c, t) for n, (c, t) in rows.items() if tag in n]
        if hit:
            sec = sum(t for _, _, t in hit) / sum(c for _, c, _ in hit) * 1e-9
            summary[tag] = dict(bytes_from_shapes=nbytes, mean_us=round(sec * 1e6, 3), bytes_per_s=round(nbytes / sec, 1),
                                share_of_hbm_peak=round(nbytes / sec / HBM_PEAK_BYTES_PER_S, 4))
    with open(out_path) as f:
        out = json.load(f)
    out["kernel_trace"] = dict(shape=dict(B=B, L=L, heads=nh, dtype="fp32", dropout=0.1), reps=TRACE_REPS, kernels=kernels, row0=summary,
                               hbm_peak_bytes_per_s=HBM_PEAK_BYTES_PER_S)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["kernel_trace"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_tower.json"))
    ap.add_argument("--trace-call", action="store_true")
    ap.add_argument("--fold-stats", default=None)
    a = ap.parse_args()
    if a.fold_stats:
        return fold_stats(a.fold_stats, a.out)
    import torch
    assert torch.cuda.is_available(), "bench_tower.py times the GPU; there is no CPU measurement"
    if a.trace_call:
        return trace_call()
    assert a.rounds >= 5, "at least five rounds, every round kept"
    out = dict(what="a whole training step of RobertaDot_NLL_LN (first-rows-only last layer) against the parent's composition (full last "
                    "layer + torch head): 12 layers, 3 calls, triplet objective, backward, Lamb(max_grad_norm=1.0), dropout 0.1",
               device=torch.cuda.get_device_name(0), torch=torch.__version__, rounds=a.rounds, steps_per_window=a.steps, warmup=a.warmup,
               note="one process, variants alternated, every round kept; fp16 rows run without a GradScaler")
    out["whole_step"] = bench(a.rounds, a.steps, a.warmup)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
