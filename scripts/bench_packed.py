"""Times a WHOLE training step of RobertaDot_NLL_LN over packed token rows (model.set_packed_rows) against the
padded step it replaces -- the same class with set_packed_rows() never called -- by the method of scripts/bench_tower.py: ONE process,
the variants alternated --rounds times, every round kept, the median reported.  12 layers at RoBERTa-base width, seeded weights,
dropout 0.1, three tower calls + the triplet objective + backward + Lamb(max_grad_norm=1.0), at bench_tower.py's shapes B x (Lq, Ld,
Ld) = 8 x (64, 512, 512) and 32 x (64, 128, 128); fp32, and torch.autocast(fp16) with precision="half" (no GradScaler); eager (device
dropout stream) and replayed from one captured graph.

Lengths: bench_tower.py's draw (uniform in L/2 .. L: three quarters of the rows carry a token) and, as a second set of legs, a
short draw (uniform in L/10 .. L/5: about a sixth, what padding MS MARCO passages of ~75 tokens to 512 gives).  N_BATCHES batches are
drawn per leg; every step copies the next one into the static inputs (both variants pay the copies), and the packed capacities are
the largest totals over the drawn batches: R_query over the query calls, R_body over the positive and negative calls.
Per leg: wall ms per step, the kernel launches and copies of one traced step, peak memory of a step; per shape the valid-row
fraction and the capacities.  A last block times torch's F.linear forward + backward alone at a BertLayer's three Linear shapes by
row count (gemm_rows_probe): what the matrix work costs at B * L rows, at the capacities drawn and at the multiples of 256 around
them.  Nothing is asserted about the times: the JSON holds what was measured."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_tower import CFG, SHAPES, peak_memory, traced, window  # noqa: E402

N_BATCHES = 4
DRAWS = {"half_to_full": (2, 1), "tenth_to_fifth": (10, 5)}   # lengths uniform in L // a .. L // b


def batches(B, lens3, vocab, gen, draw):
    """N_BATCHES x [ids, mask] * 3 and the totals per call."""
    import torch
    lo, hi = DRAWS[draw]
    out, totals = [], []
    for _ in range(N_BATCHES):
        one, tot = [], []
        for L in lens3:
            ids = torch.randint(2, vocab, (B, L), device="cuda:0", generator=gen)
            lens = torch.randint(max(1, L // lo), L // hi + 1, (B,), device="cuda:0", generator=gen)
            mask = (torch.arange(L, device="cuda:0")[None, :] < lens[:, None]).long()
            one += [ids * mask + (1 - mask), mask]
            tot.append(int(lens.sum()))
        out.append(one)
        totals.append(tot)
    return out, totals


def make_leg(variant, graph, sd, B, lens3, half, draw):
    import torch
    import lamb_util as U
    import train_step_util as S
    from ance_amd import attention as T
    from ance_amd import model
    from ance_amd.loss import nll_loss
    from ance_amd.optim import Lamb
    precision = "half" if half else "fp32"
    config = model.TowerConfig(S.VOCAB, CFG["H"], CFG["N"], CFG["inter"], S.MAX_POS, 1, CFG["eps"], CFG["pad"], 0.1, 0.1)
    m = model.RobertaDot_NLL_LN(config, precision=precision).to("cuda:0").train()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    drawn, totals = batches(B, lens3, S.VOCAB, torch.Generator(device="cuda:0").manual_seed(5), draw)
    caps = (max(t[0] for t in totals), max(max(t[1:]) for t in totals))
    if variant == "packed":
        m.set_packed_rows(query=caps[0], body=caps[1])
    named = list(m.named_parameters())
    groups = [dict(params=[q for n, q in named if S.group_of(n.replace("roberta.", "")) == k], lr=U.GROUPS[k]["lr"],
                   weight_decay=U.GROUPS[k]["weight_decay"]) for k in range(len(U.GROUPS))]
    opt = Lamb(groups, lr=1e-3, betas=U.BETAS, eps=U.EPS, max_grad_norm=1.0)
    static = [x.clone() for x in drawn[0]]
    turn = [0]

    def step():
        with torch.autocast("cuda", dtype=torch.float16, enabled=half):
            loss = nll_loss(m.query_emb(static[0], static[1]), m.body_emb(static[2], static[3]), m.body_emb(static[4], static[5]))
        loss.backward()
        opt.step()
        T.dropout_state.advance(0)

    def feed():
        turn[0] += 1
        for dst, src in zip(static, drawn[turn[0] % N_BATCHES]):
            dst.copy_(src)

    def eager():
        feed()
        step()
        opt.zero_grad(set_to_none=True)

    info = dict(valid_row_fraction=round(sum(map(sum, totals)) / (N_BATCHES * B * sum(lens3)), 4), rows_padded=[B * L for L in lens3],
                capacity_query=caps[0], capacity_body=caps[1], totals=totals)
    T.dropout_state.to_device(0)
    if not graph:
        return eager, m, info
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

    def replay():
        feed()
        g.replay()

    return replay, m, info


def bench(rounds, steps, warmup):
    import torch
    import model_util as M
    sd = M.model_state(CFG)
    res = {}
    for draw in DRAWS:
        for half in (False, True):
            for shape, (B, lens3) in SHAPES.items():
                key = "%s %s lengths %s" % ("autocast_fp16_half" if half else "fp32", shape, draw)
                legs = {"%s_%s" % (v, "graph" if g else "eager"): make_leg(v, g, sd, B, lens3, half, draw)
                        for g in (False, True) for v in ("padded", "packed")}
                seen = {name: [] for name in legs}
                for _ in range(rounds):
                    for name, (fn, _, _) in legs.items():
                        for _ in range(warmup):
                            fn()
                        seen[name].append(window(fn, steps))
                    print(key, "round", {k: round(v[-1], 3) for k, v in seen.items()}, flush=True)
                out = dict(batch=legs["packed_eager"][2])
                for name, (fn, m, _) in legs.items():
                    v = seen[name]
                    out[name] = dict(wall_ms_per_step=dict(median=round(statistics.median(v), 4), rounds=[round(x, 4) for x in v]),
                                     traced_step=traced(fn), peak_bytes_of_a_step=peak_memory(fn),
                                     packed_dropped=None if m.packed_dropped is None else int(m.packed_dropped))
                for mode in ("eager", "graph"):
                    a, b = out["padded_" + mode]["wall_ms_per_step"], out["packed_" + mode]["wall_ms_per_step"]
                    out["packed_over_padded_" + mode] = dict(ratio_of_medians=round(b["median"] / a["median"], 4),
                                                             padded_spread_ms=round(max(a["rounds"]) - min(a["rounds"]), 4),
                                                             packed_spread_ms=round(max(b["rounds"]) - min(b["rounds"]), 4))
                res[key] = out
                del legs
                torch.cuda.empty_cache()
    return res


PROBE_ROWS = (4096, 3840, 3593, 3584, 768, 683)   # B * L, the capacities of the two draws at 8 x 512, and multiples of 256 near them
PROBE_LAYERS = ((768, 768), (3072, 768), (768, 3072))   # (out, in) of a BertLayer's Linears


def gemm_rows_probe(rounds=5, iters=20):
    """torch's F.linear forward + backward (dx and dW) at a BertLayer's three Linear shapes over M rows: what a step's matrix work
    costs at the padded row count, at a packed capacity as drawn and at the multiples of 256 around it.  us per call, median."""
    import torch
    out = {}
    for dtype, name in ((torch.float32, "fp32"), (torch.float16, "fp16")):
        for n_out, n_in in PROBE_LAYERS:
            w = torch.randn(n_out, n_in, device="cuda:0", dtype=dtype, requires_grad=True)
            for M in PROBE_ROWS:
                x = torch.randn(M, n_in, device="cuda:0", dtype=dtype, requires_grad=True)
                g = torch.randn(M, n_out, device="cuda:0", dtype=dtype)

                def call():
                    torch.nn.functional.linear(x, w).backward(g)
                    x.grad = w.grad = None

                for _ in range(5):
                    call()
                v = [window(call, iters) * 1e3 for _ in range(rounds)]
                out["%s %dx%d M=%d" % (name, n_out, n_in, M)] = round(statistics.median(v), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_packed.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_packed.py times the GPU; there is no CPU measurement"
    assert a.rounds >= 5, "at least five rounds, every round kept"
    out = dict(what="a whole training step of RobertaDot_NLL_LN over packed token rows (set_packed_rows with int capacities) against the "
                    "padded step: 12 layers, 3 calls, triplet objective, backward, Lamb(max_grad_norm=1.0), dropout 0.1",
               device=torch.cuda.get_device_name(0), torch=torch.__version__, rounds=a.rounds, steps_per_window=a.steps, warmup=a.warmup,
               note="one process, variants alternated, every round kept; every step copies the next of %d drawn batches into the static "
                    "inputs; fp16 rows run without a GradScaler" % N_BATCHES)
    out["whole_step"] = bench(a.rounds, a.steps, a.warmup)
    out["linear_fwd_bwd_us_by_rows"] = gemm_rows_probe()
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
