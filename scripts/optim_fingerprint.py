#!/usr/bin/env python
"""SHA-256 fingerprints of everything the fused optimizer steps write (ance_amd.optim.Lamb, AdamW -> csrc/lamb.hip, adamw.hip,
multi_tensor.hip): the check that a restructuring of the steps moved no bit.

    python scripts/optim_fingerprint.py                                  # the library in the tree (or ANCE_AMD_LIB)
    python scripts/optim_fingerprint.py --libs PARENT.so NEW.so --out F  # one fresh child process per library; exit 1 unless they agree

Fixture: tests/adamw_util.py's (tests/lamb_util.py's sizes 0, 1, 3, 1023, 4097, 768 x 768, a zero tensor, a zero gradient, a None
gradient, two groups, plus ``late``) and the unaligned tensors of tests/test_gpu_optim_unaligned.py in the same call, three steps.
After every step the raw bytes of every tensor's p, m, v, step (one digest per tensor), of the rows of LAMB's out, of last_grad_norm
and of skipped_steps are hashed.
Runs: LAMB plain, adam=True, clipped, amp (scale 1000, clipped), amp with the second step flagged; AdamW cb, nocb, clipped, amp
(scale 3000, clipped), amp with the second step flagged.  A NaN in a parameter fails the run.

The values of the *_workspace_bytes functions at three sizes are recorded apart: between PARENT and NEW AdamW's must be equal and
LAMB's may grow by the one pointer a tensor row gained (56 -> 64 bytes per row, the table rounded to 16), by nothing else."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEPS = 3
MAX_NORM = 1.0
WORKSPACE_AT = [(1, 1, 0), (10, 2, 606000), (203, 14, 125000000)]
# name -> (optimizer, its arguments, grad_scale, the steps whose found_inf is 1 (None: no found_inf at all))
RUNS = {
    "lamb/plain": ("lamb", dict(), None, None),
    "lamb/adam": ("lamb", dict(adam=True), None, None),
    "lamb/clip": ("lamb", dict(max_grad_norm=MAX_NORM), None, None),
    "lamb/amp": ("lamb", dict(max_grad_norm=MAX_NORM), 1000.0, ()),
    "lamb/amp_flagged": ("lamb", dict(max_grad_norm=MAX_NORM), 1000.0, (1,)),
    "adamw/cb": ("adamw", dict(), None, None),
    "adamw/nocb": ("adamw", dict(correct_bias=False), None, None),
    "adamw/clip": ("adamw", dict(max_grad_norm=MAX_NORM), None, None),
    "adamw/amp": ("adamw", dict(max_grad_norm=MAX_NORM), 3000.0, ()),
    "adamw/amp_flagged": ("adamw", dict(max_grad_norm=MAX_NORM), 3000.0, (1,)),
}


def fingerprints():
    import numpy as np
    import torch
    from ance_amd import _lib
    from ance_amd.optim import AdamW, Lamb
    import adamw_util as W
    import test_gpu_optim_unaligned as X

    out = {}

    def record(name, *tensors):
        h = hashlib.sha256()
        for t in tensors:
            if isinstance(t, torch.Tensor):
                t = t.detach().contiguous().cpu().numpy()
            h.update(np.ascontiguousarray(t).tobytes())
        out[name] = h.hexdigest()

    for run, (kind, kw, scale, flagged) in RUNS.items():
        P = W.init_params()
        params = {n: torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(P[n], np.float32)).to(W.DEV)) for n in W.NAMES}
        params.update({n: torch.nn.Parameter(X._placed(X.init(n), up)) for n, _, _, up, _ in X.SPEC})
        group_of = dict(W.GROUP_OF, **X.GROUP_OF)
        groups = [dict(params=[params[n] for n in params if group_of[n] == k], lr=W.GROUPS[k]["lr"],
                       weight_decay=W.GROUPS[k]["weight_decay"]) for k in range(len(W.GROUPS))]
        opt = (Lamb if kind == "lamb" else AdamW)(groups, lr=1e-3, betas=W.BETAS, eps=W.EPS, **kw)
        for t in range(STEPS):
            W.set_lr(opt, t)
            for n in W.NAMES:
                g = W.grad(n, t)
                params[n].grad = None if g is None else torch.from_numpy(g if scale is None else g * np.float32(scale)).to(W.DEV)
            for n, _, _, _, ug in X.SPEC:
                g = X.grad(n, t)
                params[n].grad = X._placed(g if scale is None else g * np.float32(scale), ug)
            if scale is not None:
                W.set_amp(opt, grad_scale=scale, found_inf=1.0 if t in flagged else 0.0)
            opt.step()
            torch.cuda.synchronize()
            for n, p in params.items():
                at = "%s/step%d/%s" % (run, t, n)
                assert not bool(torch.isnan(p).any()), at + ": NaN"
                st = opt.state.get(p)
                if st:   # one digest over p, m, v, step
                    record(at, p, st["exp_avg"], st["exp_avg_sq"], st["step"] if isinstance(st["step"], torch.Tensor) else np.int64(st["step"]))
                else:
                    record(at, p)
            if kind == "lamb":
                record("%s/step%d/out" % (run, t), opt._prev_out[0])
            if opt.last_grad_norm is not None:
                record("%s/step%d/last_grad_norm" % (run, t), opt.last_grad_norm)
            if opt.skipped_steps is not None:
                record("%s/step%d/skipped_steps" % (run, t), opt.skipped_steps)

    L = _lib.lib()
    sizes = {}
    for n, g, total in WORKSPACE_AT:
        at = "(%d, %d, %d)" % (n, g, total)
        for fn in ("ance_lamb_workspace_bytes", "ance_lamb_clipped_workspace_bytes", "ance_lamb_amp_workspace_bytes"):
            sizes["%s%s" % (fn, at)] = int(getattr(L, fn)(n, g, total))
        for clip in (0, 1):
            sizes["ance_adamw_workspace_bytes%s clip=%d" % (at, clip)] = int(L.ance_adamw_workspace_bytes(n, g, total, clip))
    return dict(hashes=out, workspace_bytes=sizes)


def workspace_unequal(parent, new):
    """The sizes that differ by more than LAMB's tensor rows growing from 56 to 64 bytes."""
    align16 = lambda b: (b + 15) & ~15
    bad = []
    for k in sorted(set(parent) | set(new)):
        n = int(k[k.index("(") + 1:k.index(",")])
        allowed = (0, align16(64 * n) - align16(56 * n)) if k.startswith("ance_lamb") else (0,)
        if k not in parent or k not in new or new[k] - parent[k] not in allowed:
            bad.append(k)
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs="+", help="PARENT.so NEW.so ...: ANCE_AMD_LIB of one fresh child process each")
    ap.add_argument("--out", help="write the result as JSON")
    ap.add_argument("--timeout", type=int, default=300, help="seconds each child process may take")
    a = ap.parse_args()
    if not a.libs:
        res = fingerprints()
    else:
        got = {}
        for lib in a.libs:
            env = dict(os.environ, ANCE_AMD_LIB=os.path.abspath(lib))
            p = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__)], env=env,
                               stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:
                sys.exit("fingerprint run of %s failed (%d)" % (lib, p.returncode))   # nothing more is started after a failure
            got[lib] = json.loads(p.stdout.strip().splitlines()[-1])
        first = got[a.libs[0]]
        # the first library's hashes in full; of the others only what differs
        res = dict(libs=a.libs, hashes=first["hashes"], workspace_bytes={lib: got[lib]["workspace_bytes"] for lib in a.libs})
        res["unequal"] = {lib: {k: got[lib]["hashes"].get(k) for k in sorted(set(first["hashes"]) | set(got[lib]["hashes"]))
                                if first["hashes"].get(k) != got[lib]["hashes"].get(k)} for lib in a.libs[1:]}
        res["workspace_unequal"] = {lib: workspace_unequal(first["workspace_bytes"], got[lib]["workspace_bytes"]) for lib in a.libs[1:]}
    text = json.dumps(res, indent=1, sort_keys=True) if a.out else json.dumps(res, sort_keys=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    if a.libs and (any(res["unequal"].values()) or any(res["workspace_unequal"].values())):
        sys.exit(1)


if __name__ == "__main__":
    main()
