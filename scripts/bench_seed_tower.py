"""Times a WHOLE training step of SEEDEncoderDot_NLL_LN (ance_amd/model.py) against its RoBERTa twin -- the
parent's RobertaDot_NLL_LN with the same weights under HF names and a zero segment row, set_packed_rows at the same capacities, fed the
torch-compacted right-padded batch -- by the method of scripts/bench_packed.py: ONE process, the two models alternated --rounds
times, every round kept, the median reported.  12 layers, seeded weights, dropout 0.1, three tower calls + the triplet objective +
backward + Lamb(max_grad_norm=1.0), at B x (Lq, Ld, Ld) = 8 x (64, 512, 512) and 32 x (64, 128, 128); fp32, and torch.autocast(fp16)
with precision="half" (no GradScaler); eager (device dropout stream) and replayed from one captured graph.

The batches: lengths uniform in L/2 .. L, then pad ids planted strictly inside the records at 5 % of the tokens.  The SEED model
takes the [B, L] ids as they are (it packs by id: three launches); the twin takes the compacted ids and their mask (it packs by
length: two launches).  Both run the same arithmetic over the same rows, so the expectation is a ratio of 1 within the twin's own
round-to-round spread.  N_BATCHES batches are drawn per shape; every step copies the next one into the static inputs (both models pay
the copies), and the capacities are the largest non-pad totals over the drawn batches.  Per leg: wall ms per step, the kernel
launches and copies of one traced step; per shape the traced launches of the two packs alone.  Every model, optimizer and captured
graph is held to the end of the process.  Nothing is asserted about the times: the JSON holds what was measured."""
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

N_BATCHES, PAD, PAD_FRACTION = 4, 1, 0.05
KEEP = []   # every model, optimizer, graph and static input of the process: a captured step outlives nothing it reads


def compact(ids):
    import torch
    order = torch.sort((ids == PAD).to(torch.int8), dim=1, stable=True).indices
    lens = (ids != PAD).sum(1)
    return ids.gather(1, order), (torch.arange(ids.shape[1], device=ids.device)[None, :] < lens[:, None]).long()


def batches(B, lens3, vocab, gen):
    """N_BATCHES x (the SEED model's [ids, None] * 3, the twin's [compacted ids, mask] * 3) and the non-pad totals per call."""
    import torch
    seed_in, twin_in, totals = [], [], []
    for _ in range(N_BATCHES):
        a, b, tot = [], [], []
        for L in lens3:
            ids = torch.randint(2, vocab, (B, L), device="cuda:0", generator=gen)
            lens = torch.randint(max(1, L // 2), L + 1, (B,), device="cuda:0", generator=gen)
            col = torch.arange(L, device="cuda:0")[None, :]
            inside = (col >= 1) & (col < lens[:, None] - 1) & (torch.rand((B, L), device="cuda:0", generator=gen) < PAD_FRACTION)
            ids = torch.where((col >= lens[:, None]) | inside, torch.full_like(ids, PAD), ids)
            a += [ids, None]
            b += list(compact(ids))
            tot.append(int((ids != PAD).sum()))
        seed_in.append(a)
        twin_in.append(b)
        totals.append(tot)
    return seed_in, twin_in, totals


def make_leg(variant, graph, sd_hf, drawn, caps, half):
    import torch
    import seed_util
    from ance_amd import attention as T
    from ance_amd import model
    from ance_amd.optim import Lamb
    precision = "half" if half else "fp32"
    if variant == "seed":
        sd = {k: torch.from_numpy(v) for k, v in seed_util.to_seed_names(sd_hf).items()}
        m = model.SEEDEncoderDot_NLL_LN.from_state_dict(sd, precision=precision, dropout=0.1)
    else:
        m = model.RobertaDot_NLL_LN.from_state_dict({k: torch.from_numpy(v) for k, v in sd_hf.items()}, precision=precision, dropout=0.1)
    m = m.to("cuda:0").train().set_packed_rows(query=caps[0], body=caps[1])
    no_decay = ("bias", "LayerNorm.weight")   # the reference's grouping, by name
    named = list(m.named_parameters())
    groups = [dict(params=[p for n, p in named if not any(nd in n for nd in no_decay)], weight_decay=0.01),
              dict(params=[p for n, p in named if any(nd in n for nd in no_decay)], weight_decay=0.0)]
    opt = Lamb(groups, lr=1e-3, eps=1e-6, max_grad_norm=1.0)
    static = [None if x is None else x.clone() for x in drawn[0]]
    turn = [0]

    def step():
        with torch.autocast("cuda", dtype=torch.float16, enabled=half):
            loss = m(*static)[0]
        loss.backward()
        opt.step()
        T.dropout_state.advance(0)

    def feed():
        turn[0] += 1
        for dst, src in zip(static, drawn[turn[0] % N_BATCHES]):
            if dst is not None:
                dst.copy_(src)

    def eager():
        feed()
        step()
        opt.zero_grad(set_to_none=True)

    KEEP.append((m, opt, static, drawn, step, feed, eager))
    T.dropout_state.to_device(0)
    if not graph:
        return eager, m
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

    KEEP.append((g, side, replay))
    return replay, m


def pack_launches(seed_in, twin_in, caps):
    """The traced launches of the two packs alone, at the body capacity: int32 ids and a counter made beforehand, so that no torch
    kernel (the int64 -> int32 cast of the ids, the fill of a fresh counter) is counted with them."""
    import torch
    from ance_amd.attention import lens_from_mask
    from ance_amd.packing import pack_tokens, pack_tokens_by_id
    import train_step_util as S
    ids, comp, mask = seed_in[0][2].to(torch.int32), twin_in[0][2].to(torch.int32), twin_in[0][3]
    lens, counter = lens_from_mask(mask).to(torch.int32), torch.zeros((), dtype=torch.int64, device=ids.device)
    return dict(pack_tokens_by_id=traced(lambda: pack_tokens_by_id(ids, caps[1], PAD, S.VOCAB, S.MAX_POS, counter)),
                pack_tokens=traced(lambda: pack_tokens(comp, lens, caps[1], None, "roberta", PAD, S.VOCAB, S.MAX_POS, counter)))


def bench(rounds, steps, warmup):
    import numpy as np
    import torch
    import model_util as M
    import train_step_util as S
    sd_hf = dict(M.model_state(CFG))
    seg = "roberta.embeddings.token_type_embeddings.weight"
    sd_hf[seg] = np.zeros_like(sd_hf[seg])   # SEED has no segment table: the twin adds a zero row
    res = {}
    for half in (False, True):
        for shape, (B, lens3) in SHAPES.items():
            key = "%s %s" % ("autocast_fp16_half" if half else "fp32", shape)
            seed_in, twin_in, totals = batches(B, lens3, S.VOCAB, torch.Generator(device="cuda:0").manual_seed(5))
            caps = (max(t[0] for t in totals), max(max(t[1:]) for t in totals))
            legs = {"%s_%s" % (v, "graph" if g else "eager"): make_leg(v, g, sd_hf, seed_in if v == "seed" else twin_in, caps, half)
                    for g in (False, True) for v in ("twin", "seed")}
            seen = {name: [] for name in legs}
            for _ in range(rounds):
                for name, (fn, _) in legs.items():
                    for _ in range(warmup):
                        fn()
                    seen[name].append(window(fn, steps))
                print(key, "round", {k: round(v[-1], 3) for k, v in seen.items()}, flush=True)
            out = dict(batch=dict(rows_padded=[B * L for L in lens3], capacity_query=caps[0], capacity_body=caps[1], totals=totals,
                                  non_pad_fraction=round(sum(map(sum, totals)) / (N_BATCHES * B * sum(lens3)), 4)),
                       pack_alone_traced=pack_launches(seed_in, twin_in, caps))
            for name, (fn, m) in legs.items():
                v = seen[name]
                out[name] = dict(wall_ms_per_step=dict(median=round(statistics.median(v), 4), rounds=[round(x, 4) for x in v]),
                                 traced_step=traced(fn), peak_bytes_of_a_step=peak_memory(fn), packed_dropped=int(m.packed_dropped))
            for mode in ("eager", "graph"):
                a, b = out["twin_" + mode]["wall_ms_per_step"], out["seed_" + mode]["wall_ms_per_step"]
                out["seed_over_twin_" + mode] = dict(ratio_of_medians=round(b["median"] / a["median"], 4),
                                                     twin_spread_ms=round(max(a["rounds"]) - min(a["rounds"]), 4),
                                                     seed_spread_ms=round(max(b["rounds"]) - min(b["rounds"]), 4),
                                                     launches_seed_minus_twin=out["seed_" + mode]["traced_step"]["kernel_launches"]
                                                     - out["twin_" + mode]["traced_step"]["kernel_launches"])
            res[key] = out
            torch.cuda.synchronize()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_seed_tower.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_seed_tower.py times the GPU; there is no CPU measurement"
    assert a.rounds >= 5, "at least five rounds, every round kept"
    out = dict(what="a whole training step of SEEDEncoderDot_NLL_LN (packed by id) against its RoBERTa twin (RobertaDot_NLL_LN, the same "
                    "weights, packed by length on the compacted batch, the same capacities): 12 layers, 3 calls, triplet objective, "
                    "backward, Lamb(max_grad_norm=1.0), dropout 0.1, interior pads at 5 % of the tokens",
               device=torch.cuda.get_device_name(0), torch=torch.__version__, rounds=a.rounds, steps_per_window=a.steps, warmup=a.warmup,
               note="one process, the two models alternated, every round kept; every step copies the next of %d drawn batches into the "
                    "static inputs; fp16 rows run without a GradScaler; every captured object lives to the end of the process" % N_BATCHES)
    out["whole_step"] = bench(a.rounds, a.steps, a.warmup)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
