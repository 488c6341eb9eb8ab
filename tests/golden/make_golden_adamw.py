"""Generates tests/golden/adamw.npz and adamw.json:

    python tests/golden/make_golden_adamw.py

transformers 2.3.0 (the reference's pin, setup.py:20) is not installable beside the transformers this project is developed against,
and later versions no longer have the class.  So ``AdamW230`` below restates transformers 2.3.0 optimization.py, class AdamW
(__init__ and step), line by line with torch fp32 ops on the CPU -- the form make_golden_objective.py uses for the in-batch lines
of drivers/run_ann_dpr.py.  The only edits are the keyword spellings current torch wants (add_(x, alpha=a) for add_(a, x),
addcmul_(x, y, value=a), addcdiv_(x, y, value=a)): the arithmetic and its order are 2.3.0's.

Runs on tests/adamw_util.py's fixture (adamw_util.RUNS): five steps with correct_bias, three without, and three steps each of
torch.nn.utils.clip_grad_norm_ + step for a max_grad_norm that clips every step and one that never does, the learning rate
changing every step.  Recorded after every step: p, m, v of every parameter that has state (the 768 x 768 tensor at every
SAMPLE_STRIDE-th element; m and v do not depend on the step size, so the runs of adamw_util.MV_AS do not repeat them), beside
each its max |delta| from the fp64 restatement (adamw_util.run_fp64) as ``<key>.ref_err``, the total norm clip_grad_norm_
returned, and state_dict()'s layout: per run the keys, value types and param_groups once, per step the step counts and the
learning rates (adamw_util.layout_at puts a step's state_dict layout together again)."""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import adamw_util as W  # noqa: E402
import lamb_util as U  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


class AdamW230(torch.optim.Optimizer):
    """transformers 2.3.0, optimization.py, class AdamW."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, correct_bias=True):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {} - should be >= 0.0".format(lr))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[1]))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {} - should be >= 0.0".format(eps))
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, correct_bias=correct_bias)
        super().__init__(params, defaults)

    def step(self, closure=None):
        loss = None
        if closure is not None:
            loss = closure()
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                grad = p.grad.data
                if grad.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = 0
                    state["exp_avg"] = torch.zeros_like(p.data)
                    state["exp_avg_sq"] = torch.zeros_like(p.data)
                exp_avg, exp_avg_sq = state["exp_avg"], state["exp_avg_sq"]
                beta1, beta2 = group["betas"]
                state["step"] += 1
                exp_avg.mul_(beta1).add_(grad, alpha=1.0 - beta1)
                exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1.0 - beta2)
                denom = exp_avg_sq.sqrt().add_(group["eps"])
                step_size = group["lr"]
                if group["correct_bias"]:
                    bias_correction1 = 1.0 - beta1 ** state["step"]
                    bias_correction2 = 1.0 - beta2 ** state["step"]
                    step_size = step_size * math.sqrt(bias_correction2) / bias_correction1
                p.data.addcdiv_(exp_avg, denom, value=-step_size)
                if group["weight_decay"] > 0.0:
                    p.data.add_(p.data, alpha=-group["lr"] * group["weight_decay"])
        return loss


def run(name):
    steps, correct_bias, max_norm = W.RUNS[name]
    P = W.init_params()
    params = {n: torch.nn.Parameter(torch.from_numpy(P[n].copy())) for n in W.NAMES}
    groups = [dict(params=[params[n] for n in W.NAMES if W.GROUP_OF[n] == k], lr=W.GROUPS[k]["lr"],
                   weight_decay=W.GROUPS[k]["weight_decay"]) for k in range(len(W.GROUPS))]
    opt = AdamW230(groups, lr=1e-3, betas=W.BETAS, eps=W.EPS, correct_bias=correct_bias)
    traj = W.run_fp64(steps, correct_bias, max_norm)
    rec, steps_tab, lr_tab = {}, [], []
    for t in range(steps):
        W.set_lr(opt, t)
        for n in W.NAMES:
            g = W.grad(n, t)
            params[n].grad = None if g is None else torch.from_numpy(g.copy())
        if max_norm is not None:
            total = torch.nn.utils.clip_grad_norm_([p for p in params.values()], max_norm)
            rec["%d.total_norm" % t] = np.array(float(total), np.float32)
        opt.step()
        for n in W.NAMES:
            st = opt.state.get(params[n], {})  # .get: the defaultdict must not grow an entry
            if not st:
                continue
            for key, x, ix in (("p", params[n].detach(), 0), ("m", st["exp_avg"], 1), ("v", st["exp_avg_sq"], 2)):
                if key != "p" and name in W.MV_AS:
                    continue
                k = "%s.%d.%s" % (n, t, key)
                rec[k] = U.recorded(n, x.numpy())
                rec[k + ".ref_err"] = np.array(np.abs(rec[k].astype(np.float64) - U.recorded(n, traj[t][2][n][ix])).max(initial=0.0))
        sd = opt.state_dict()
        # one layout per run (the key types and param_groups never change) and, per step, what does: the step counts and the rates
        layout = dict(state_types={str(i): {k: type(v).__name__ for k, v in sorted(s.items())} for i, s in sd["state"].items()},
                      param_groups=[{k: (list(v) if isinstance(v, tuple) else v) for k, v in g.items() if k != "lr"}
                                    for g in sd["param_groups"]])
        steps_tab.append({str(i): s["step"] for i, s in sd["state"].items()})
        lr_tab.append([g["lr"] for g in sd["param_groups"]])
    layouts = dict(layout, step=steps_tab, lr=lr_tab)
    return rec, layouts


def main():
    arrays, layouts = {}, {}
    for name in W.RUNS:
        rec, layouts[name] = run(name)
        arrays.update({"%s.%s" % (name, k): v for k, v in rec.items()})
    np.savez_compressed(os.path.join(OUT, "adamw.npz"), **arrays)
    meta = dict(generator="tests/golden/make_golden_adamw.py",
                reference="transformers 2.3.0 optimization.py AdamW, restated (CPU fp32, torch %s)" % torch.__version__,
                runs={k: dict(steps=v[0], correct_bias=v[1], max_grad_norm=v[2]) for k, v in W.RUNS.items()},
                sample_stride=U.SAMPLE_STRIDE, param_order=W.PACKED, state_dict=layouts)
    with open(os.path.join(OUT, "adamw.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    errs = [float(v) for k, v in arrays.items() if k.endswith(".p.ref_err")]
    print("adamw.npz %d B, adamw.json %d B; ref_err of p: %.3g .. %.3g" % (
        os.path.getsize(os.path.join(OUT, "adamw.npz")), os.path.getsize(os.path.join(OUT, "adamw.json")), min(errs), max(errs)))


if __name__ == "__main__":
    main()
