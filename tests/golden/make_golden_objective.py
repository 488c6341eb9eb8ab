"""Generates tests/golden/objective.npz and objective.json by running the REAL reference (imported through oracle/ref_harness.py)
on CPU fp32 in the build container:

    python tests/golden/make_golden_objective.py

* NLL.forward, NLL_MultiChunk.forward and BiEncoder.forward's triplet branch (model/models.py:57-81, 84-134, 260-271) with stub
  towers that return leaf tensors, so loss.backward() yields the reference's own gradients of q, a, b.  MaxP: 4 chunks, rows whose
  trailing chunks are masked, rows with every chunk but 0 masked and rows where two chunks are exact duplicates; what torch's
  max backward does with that tie is recorded (``maxp_tie``).
* The in-batch objective of drivers/run_ann_dpr.py:356-365.  The driver cannot be imported here (it pulls in the whole trainer and
  its distributed set-up), so those ten lines are restated below with torch, cited in objective.json.
* Three steps of torch.nn.utils.clip_grad_norm_ + the reference's utils/lamb.py Lamb on tests/lamb_util.py's parameter set, for a
  max_grad_norm that clips at every step and one that never does.
* Beside every fp32 result its max |delta| from the fp64 restatement (tests/objective_util.py) over the FULL tensor (``ref_err``):
  the reference's own distance from fp64.  Inputs are not stored (tests regenerate them from oracle.encoder_ref.det_normal);
  tensors above 30,000 elements are recorded at every 13th element."""
import importlib
import json
import os
import sys
import types
import warnings

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness  # noqa: E402
import lamb_util as U  # noqa: E402
import objective_util as O  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def leaf(x):
    return torch.from_numpy(np.array(x)).requires_grad_(True)


def record(arrays, meta, case, loss, grads, want):
    """grads / want: {name: reference fp32 tensor / fp64 array}."""
    meta[case] = dict(loss=float(loss), loss_fp64=want["loss"], ref_err={}, scale={})
    for k, g in grads.items():
        g = g.detach().numpy()
        arrays["%s.%s" % (case, k)] = O.recorded(g)
        meta[case]["ref_err"][k] = float(np.abs(g.astype(np.float64) - want[k]).max())
        meta[case]["scale"][k] = float(np.abs(want[k]).max())


def triplets(ref, arrays, meta):
    for case in list(O.FIRSTP_CASES) + list(O.DPR_TRIPLET_CASES) + ["maxp"]:
        q, a, b, ma, mb = O.triplet_inputs(case)
        tq, ta, tb = leaf(q), leaf(a), leaf(b)
        n = q.shape[0]
        ids = torch.zeros((n, 2), dtype=torch.long)
        if case == "maxp":
            # body_emb sees the ids of a or b: tell them apart by their first entry; base_len 2 -> chunk_factor = 8 // 2
            stub = types.SimpleNamespace(base_len=2, query_emb=lambda i, m: tq, body_emb=lambda i, m: ta if int(i[0, 0]) == 1 else tb)
            ids_a = torch.ones((n, 2 * O.MAXP_CHUNKS), dtype=torch.long)
            ids_b = torch.zeros((n, 2 * O.MAXP_CHUNKS), dtype=torch.long)
            att_a = torch.from_numpy(np.repeat(ma, 2, axis=1)).long()
            att_b = torch.from_numpy(np.repeat(mb, 2, axis=1)).long()
            (loss,) = ref.models.NLL_MultiChunk.forward(stub, ids, None, ids_a, att_a, ids_b, att_b)
        else:
            stub = types.SimpleNamespace(query_emb=lambda i, m: tq, body_emb=lambda i, m: ta if int(i[0, 0]) == 1 else tb)
            cls = ref.models.BiEncoder if case in O.DPR_TRIPLET_CASES else ref.models.NLL
            (loss,) = cls.forward(stub, ids, None, torch.ones((n, 2), dtype=torch.long), None, ids, None)
        loss.backward()
        want = O.nll_fp64(q, a, b, ma, mb)
        if case == "maxp":
            # the restatement's winners must be robust: the best biased score leads the next DIFFERENT one by a wide margin
            for t, m in ((a, ma), (b, mb)):
                s = (q[:, None, :].astype(np.float64) * t).sum(-1) + (1.0 - m) * -9999.0
                for row in s:
                    rest = row[row != row.max()]
                    assert rest.size == 0 or row.max() - rest.max() > 1e-3, row
            tie = {}
            for name, g, (r, c0, c1) in (("a", ta.grad, O.MAXP_DUP["a"]), ("b", tb.grad, O.MAXP_DUP["b"])):
                nz = [c for c in range(O.MAXP_CHUNKS) if float(g[r, c].abs().max()) > 0]
                assert int(want["c" + name][r]) == c0 and set(nz) <= {c0, c1}, (name, nz)
                tie[name] = dict(row=r, duplicates=[c0, c1], torch_gradient_at=nz)
            meta["maxp_tie"] = dict(tie, rule_tested="the lowest index" if all(v["torch_gradient_at"] == [v["duplicates"][0]]
                                                                               for v in tie.values()) else "fp64 restatement only")
        record(arrays, meta, case, loss, dict(gq=tq.grad, ga=ta.grad, gb=tb.grad), want)


def inbatch(arrays, meta):
    meta["inbatch_source"] = ("drivers/run_ann_dpr.py:356-365 restated (the driver module cannot be imported without its trainer "
                              "environment): scores = matmul(q, ctx^T); log_softmax(dim=1); F.nll_loss(..., positive_idx, "
                              "reduction='mean'); correct = (argmax == positive_idx).sum()")
    for case, nq in O.INBATCH_CASES.items():
        q, ctx, pos = O.inbatch_inputs(nq)
        margins = O.inbatch_margins(q, ctx, pos)
        assert margins.min() > 1e-3, margins.min()
        tq, tc = leaf(q), leaf(ctx)
        scores = torch.matmul(tq, torch.transpose(tc, 0, 1)).view(nq, -1)
        softmax_scores = F.log_softmax(scores, dim=1)
        loss = F.nll_loss(softmax_scores, torch.from_numpy(pos), reduction='mean')
        _, max_idxs = torch.max(softmax_scores, 1)
        n_correct = int((max_idxs == torch.from_numpy(pos)).sum())
        loss.backward()
        want = O.inbatch_fp64(q, ctx, pos)
        record(arrays, meta, case, loss, dict(gq=tq.grad, gctx=tc.grad), want)
        meta[case].update(n_correct_reference=n_correct, n_correct_fp64=want["n_correct"], min_margin_fp64=float(margins.min()))
        arrays[case + ".correct"] = want["correct"]


def lamb_clipped(arrays, meta):
    Lamb = importlib.import_module("utils.lamb").Lamb
    for run, max_norm in O.CLIP_RUNS.items():
        P = U.init_params()
        params = {n: torch.nn.Parameter(torch.from_numpy(P[n].copy())) for n, *_ in U.SPEC}
        groups = [dict(params=[params[n] for n, _, gi, _, _ in U.SPEC if gi == k], lr=U.GROUPS[k]["lr"],
                       weight_decay=U.GROUPS[k]["weight_decay"]) for k in range(len(U.GROUPS))]
        opt = Lamb(groups, lr=1e-3, betas=U.BETAS, eps=U.EPS)
        norms = []
        for t in range(O.CLIP_STEPS):
            for k, g in enumerate(opt.param_groups):
                g["lr"] = U.group_lr(k, t)
            for n, *_ in U.SPEC:
                gr = U.grad(n, t)
                params[n].grad = None if gr is None else torch.from_numpy(gr.copy())
            norms.append(float(torch.nn.utils.clip_grad_norm_(list(params.values()), max_norm)))
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                opt.step()
            for n, *_ in U.SPEC:
                st = opt.state.get(params[n], {})
                if not st:
                    continue
                for key, x in (("p", params[n].detach()), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"])):
                    arrays["lamb_%s.%s.%d.%s" % (run, n, t, key)] = U.recorded(n, x.numpy())
                arrays["lamb_%s.%s.%d.norms" % (run, n, t)] = np.array(
                    [float(st["weight_norm"]), float(st["adam_norm"]), float(st["trust_ratio"])], np.float32)
        want = O.run_clipped_fp64(max_norm)
        meta["lamb_" + run] = dict(max_grad_norm=max_norm, total_norm=norms, total_norm_fp64=[w[0] for w in want],
                                   coef_fp64=[w[1] for w in want])
        assert all((w[1] < 1.0) == (run == "clip") for w in want)


def main():
    ref = ref_harness.load_reference()
    arrays, meta = {}, dict(generator="tests/golden/make_golden_objective.py", torch=torch.__version__,
                            sample_stride=O.SAMPLE_STRIDE, sample_min=O.SAMPLE_MIN)
    triplets(ref, arrays, meta)
    inbatch(arrays, meta)
    lamb_clipped(arrays, meta)
    np.savez_compressed(os.path.join(OUT, "objective.npz"), **arrays)
    with open(os.path.join(OUT, "objective.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("objective.npz %d B, objective.json %d B" % tuple(os.path.getsize(os.path.join(OUT, x)) for x in ("objective.npz", "objective.json")))
    print(json.dumps({k: v for k, v in meta.items() if isinstance(v, dict)}, indent=1)[:6000])


if __name__ == "__main__":
    main()
