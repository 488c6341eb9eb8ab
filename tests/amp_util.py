"""The fused LAMB step under loss scaling (ance_amd.optim.Lamb under torch.amp.GradScaler -> ance_lamb_step_amp, csrc/lamb.hip)
restated in fp64 NumPy on tests/lamb_util.py's fixture -- the oracle of tests/test_lamb_amp.py and tests/test_gpu_lamb_amp.py -- and
the helpers the GPU tests share.

The arithmetic the kernels state: inv = float32(1 / float64(scale)), what GradScaler.unscale_ multiplies by; every gradient element
enters the step as the single fp32 product g * inv; the clipping norm is taken over those products; a step whose found_inf is not
0 changes nothing.  From the products on, the restatement is objective_util.clip_fp64 and lamb_util.step_fp64 in fp64.
"""
import numpy as np

import lamb_util as U
import objective_util as O

NAMES = [n for n, *_ in U.SPEC]
WITH_GRAD = [n for n in NAMES if U.grad(n, 0) is not None]
DEV = "cuda:0"


def inv_scale(scale):
    """float32(1 / float64(float32(scale)))"""
    return np.float32(1.0 / np.float64(np.float32(scale)))


def scaled_grad(name, t, scale):
    """What backward() of the scaled loss leaves in p.grad: the fixture's gradient times the scale, in fp32 (None: no gradient)."""
    g = U.grad(name, t)
    return None if g is None else g * np.float32(scale)


def unscaled(g, scale):
    """The fp32 products g * inv, element by element."""
    return np.asarray(g, np.float32) * inv_scale(scale)


def grad_norm_fp64(t, scale):
    """The 2-norm, in fp64, of the fp32 products the step sees at step t."""
    return O.clip_fp64([unscaled(scaled_grad(n, t, scale), scale) for n in WITH_GRAD], 1.0)[0]


def run_amp_fp64(max_norm, scale, steps=O.CLIP_STEPS, skip=()):
    """The fixture's trajectory with gradients scaled by ``scale`` in memory: [(total_norm, coef, {name: (p, m, v, wn, an, tr)})]
    per step; max_norm None: no clipping (total_norm is still reported, coef is 1).  skip: the steps (0-based) whose found_inf is
    set -- nothing changes there and the record repeats the previous one's (wn, an, tr), (0, 0, 1) when there is none."""
    P = U.init_params()
    state = {n: (P[n].astype(np.float64), np.zeros(P[n].shape), np.zeros(P[n].shape)) for n in P}
    norms = {n: (0.0, 0.0, 1.0) for n in WITH_GRAD}
    out = []
    for t in range(steps):
        grads = {n: unscaled(scaled_grad(n, t, scale), scale) for n in WITH_GRAD}
        total, coef = O.clip_fp64(list(grads.values()), 1.0 if max_norm is None else max_norm)
        if max_norm is None:
            coef = 1.0
        rec = {}
        for name, shape, gi, _, _ in U.SPEC:
            if name not in grads:
                continue
            p, m, v = state[name]
            if t in skip:
                rec[name] = (p, m, v) + norms[name]
                continue
            r = U.step_fp64(p, grads[name].astype(np.float64) * coef, m, v, U.group_lr(gi, t), U.BETAS, U.EPS,
                            U.GROUPS[gi]["weight_decay"], False)
            state[name], norms[name] = r[:3], r[3:]
            rec[name] = r
        out.append((total, coef, rec))
    return out


# ------------------------------------------------------------------------------------------------------- GPU helpers
def make(max_grad_norm=None, names=NAMES):
    """({name: Parameter on the GPU}, Lamb) on the fixture's initial values and groups."""
    import torch

    from ance_amd.optim import Lamb
    P = U.init_params()
    params = {n: torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(P[n], np.float32)).to(DEV)) for n in names}
    groups = [dict(params=[params[n] for n, _, gi, _, _ in U.SPEC if gi == k and n in params], lr=U.GROUPS[k]["lr"],
                   weight_decay=U.GROUPS[k]["weight_decay"]) for k in range(len(U.GROUPS))]
    return params, Lamb(groups, lr=1e-3, betas=U.BETAS, eps=U.EPS, max_grad_norm=max_grad_norm)


def set_grads(params, t, scale=None):
    """p.grad = the fixture's gradient of step t, times ``scale`` (a Python number: an fp32 product on the device)."""
    import torch
    for n in params:
        g = U.grad(n, t)
        if g is None:
            params[n].grad = None
        else:
            g = torch.from_numpy(g).to(DEV)
            params[n].grad = g if scale is None else g * torch.tensor(scale, dtype=torch.float32, device=DEV)


def set_lr(opt, t):
    for k, g in enumerate(opt.param_groups):
        g["lr"] = U.group_lr(k, t)


def set_amp(opt, grad_scale=None, found_inf=None):
    """What GradScaler.step attaches: 0-dim fp32 device tensors (None: the attribute is None)."""
    import torch
    opt.grad_scale = None if grad_scale is None else torch.full((), grad_scale, dtype=torch.float32, device=DEV)
    opt.found_inf = None if found_inf is None else torch.full((), found_inf, dtype=torch.float32, device=DEV)


def state(params, opt):
    """{name: [p, m, v, (wn, an, tr)]} as NumPy copies (p alone for a parameter without state)."""
    out = {}
    for n, p in params.items():
        st = opt.state.get(p, {})
        out[n] = [p.detach().cpu().numpy().copy()]
        if st:
            out[n] += [st["exp_avg"].cpu().numpy().copy(), st["exp_avg_sq"].cpu().numpy().copy(),
                       np.array([float(st["weight_norm"]), float(st["adam_norm"]), float(st["trust_ratio"])], np.float32)]
    return out


def assert_same(a, b):
    assert a.keys() == b.keys()
    for n in a:
        assert len(a[n]) == len(b[n]), n
        for x, y in zip(a[n], b[n]):
            np.testing.assert_array_equal(x, y, err_msg=n)
