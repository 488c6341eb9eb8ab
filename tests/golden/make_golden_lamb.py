"""Generates tests/golden/lamb.npz and lamb.json by running the REAL reference's Lamb (utils/lamb.py, imported through
oracle/ref_harness.py) on CPU fp32 in the build container:

    python tests/golden/make_golden_lamb.py

The fixture (tests/lamb_util.py: SPEC, GROUPS) covers tensors of 0, 1, 3, 1,023, 4,097 and 768 x 768 elements, zero biases
(wn == 0 at step 1), |p| > 10 (the clamp), an all-zero gradient (an == 0), a parameter whose gradient is None, two groups of
different lr (one with weight decay) and a learning rate that changes every step; then a second run with adam=True.
Parameters and gradients come from oracle.encoder_ref.det_normal.  Recorded after every step: p, m, v (m, v of the adam run
equal the LAMB run's and are not repeated; the 768 x 768 tensor at every SAMPLE_STRIDE-th element), wn, an, tr, and the keys,
value types and param_groups of the reference's state_dict()."""
import importlib
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness  # noqa: E402
import lamb_util as U  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def run(adam):
    ref_harness.load_reference()
    Lamb = importlib.import_module("utils.lamb").Lamb
    P = U.init_params()
    params = {n: torch.nn.Parameter(torch.from_numpy(P[n].copy())) for n, *_ in U.SPEC}
    groups = [dict(params=[params[n] for n, _, gi, _, _ in U.SPEC if gi == k], lr=U.GROUPS[k]["lr"],
                   weight_decay=U.GROUPS[k]["weight_decay"]) for k in range(len(U.GROUPS))]
    opt = Lamb(groups, lr=1e-3, betas=U.BETAS, eps=U.EPS, adam=adam)
    rec, layouts = {}, []
    for t in range(U.STEPS):
        for k, g in enumerate(opt.param_groups):
            g["lr"] = U.group_lr(k, t)
        for n, *_ in U.SPEC:
            gr = U.grad(n, t)
            params[n].grad = None if gr is None else torch.from_numpy(gr.copy())
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            opt.step()
        for n, *_ in U.SPEC:
            st = opt.state.get(params[n], {})  # .get: the defaultdict must not grow an entry
            rec["%s.%d.p" % (n, t)] = U.recorded(n, params[n].detach().numpy())
            if not st:
                continue
            if not adam:
                rec["%s.%d.m" % (n, t)] = U.recorded(n, st["exp_avg"].numpy())
                rec["%s.%d.v" % (n, t)] = U.recorded(n, st["exp_avg_sq"].numpy())
            rec["%s.%d.norms" % (n, t)] = np.array([float(st["weight_norm"]), float(st["adam_norm"]), float(st["trust_ratio"])],
                                                   np.float32)
        sd = opt.state_dict()
        layouts.append(dict(
            state={str(i): {k: type(v).__name__ for k, v in sorted(s.items())} for i, s in sd["state"].items()},
            step={str(i): s["step"] for i, s in sd["state"].items()},
            param_groups=[{k: (list(v) if isinstance(v, tuple) else v) for k, v in g.items()} for g in sd["param_groups"]]))
    return rec, layouts


def main():
    lamb, lamb_layout = run(False)
    adam, adam_layout = run(True)
    arrays = {"lamb." + k: v for k, v in lamb.items()}
    arrays.update({"adam." + k: v for k, v in adam.items()})
    np.savez_compressed(os.path.join(OUT, "lamb.npz"), **arrays)
    meta = dict(generator="tests/golden/make_golden_lamb.py", reference="utils/lamb.py Lamb (CPU fp32, torch %s)" % torch.__version__,
                steps=U.STEPS, sample_stride=U.SAMPLE_STRIDE, param_order=[n for n, *_ in U.SPEC],
                state_dict_lamb=lamb_layout, state_dict_adam=adam_layout)
    with open(os.path.join(OUT, "lamb.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    sizes = [os.path.getsize(os.path.join(OUT, x)) for x in ("lamb.npz", "lamb.json")]
    print("lamb.npz %d B, lamb.json %d B" % tuple(sizes))


if __name__ == "__main__":
    main()
