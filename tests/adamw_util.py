"""The AdamW step of transformers 2.3.0 (optimization.py, class AdamW -- the optimizer drivers/run_ann_dpr.py trains with by default)
restated in fp64 NumPy -- the oracle of tests/test_adamw.py and tests/test_gpu_adamw.py -- and the fixture both tests and
tests/golden/make_golden_adamw.py share.

One step of one tensor whose state has seen ``t - 1`` steps, the group's hyper-parameters rounded to fp32 as the fp32
implementations use them (as lamb_util.step_fp64):
    g' = g [times inv = float32(1 / float64(scale)) as an fp32 product under loss scaling, then times the clip factor]
    m <- b1 m + (1 - b1) g' ;  v <- b2 v + (1 - b2) g' g'
    ss = float32(lr sqrt(1 - b2^t) / (1 - b1^t))   (the Python doubles; float32(lr) when correct_bias is off)
    p <- p - ss m / (sqrt(v) + eps) ;  p <- p + float32(-lr wd) p on the updated p when wd > 0

The fixture is lamb_util's (sizes 0, 1, 3, 1023, 4097 and the 36-chunk 768 x 768 tensor, a zero-initialised tensor, a zero
gradient, a None gradient, two groups, one with weight decay 0.01, a learning rate that changes every step) plus ``late``: no
gradient at steps 0-1, one from step 2 -- its bias correction starts at 1 while the others are at 3.
"""
import math

import numpy as np

import lamb_util as U
import objective_util as O
from oracle.encoder_ref import det_normal

LATE_FROM = 2
SPEC = U.SPEC + [("late", (130,), 0, 0.02, 0.01)]
NAMES = [n for n, *_ in SPEC]
GROUP_OF = {n: gi for n, _, gi, _, _ in SPEC}
GROUPS, EPS, BETAS = U.GROUPS, U.EPS, U.BETAS
# the index a parameter has in state_dict(): group by group
PACKED = [n for k in range(len(U.GROUPS)) for n in NAMES if GROUP_OF[n] == k]
# name -> (steps, correct_bias, max_grad_norm): the fixture's gradient norm is ~7.7, so 1.0 clips at every step and 1000 never
RUNS = {"cb": (5, True, None), "nocb": (3, False, None), "clip": (3, True, O.CLIP_RUNS["clip"]), "noclip": (3, True, O.CLIP_RUNS["noclip"])}
# m and v read neither the step size nor, with a clip factor of 1, the clipping: these runs' are the first steps of "cb", bit for bit,
# and the golden does not repeat them
MV_AS = {"nocb": "cb", "noclip": "cb"}
DEV = "cuda:0"


def init_params():
    out = U.init_params()
    out["late"] = det_normal(7, "adamw.p.late", (130,), 0.02)
    return out


def grad(name, t):
    """The gradient of ``name`` at step t (0-based), or None."""
    if name == "late":
        return None if t < LATE_FROM else det_normal(100 + t, "adamw.g.late", (130,), 0.01)
    return U.grad(name, t)


def with_grad(t):
    return [n for n in NAMES if grad(n, t) is not None]


def step_size(lr, betas, t, correct_bias, rnd=U.f32):
    """float32 of 2.3.0's step_size for a state at its t-th step (1-based), in Python doubles as there."""
    if not correct_bias:
        return rnd(lr)
    return rnd(lr * math.sqrt(1.0 - betas[1] ** t) / (1.0 - betas[0] ** t))


def step_fp64(p, g, m, v, t, lr, betas, eps, wd, correct_bias=True, rnd=U.f32):
    """One step of one tensor in fp64; t: the state's step count after this step.  Returns (p, m, v).  rnd: how a hyper-parameter
    enters (fp32-rounded as the fp32 implementations have it; ``float`` for the plain algebra)."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    b1, b2 = betas
    m = rnd(b1) * m + rnd(1 - b1) * g
    v = rnd(b2) * v + rnd(1 - b2) * g * g
    p = p - step_size(lr, betas, t, correct_bias, rnd) * (m / (np.sqrt(v) + rnd(eps)))
    if wd > 0:
        p = p + rnd(-lr * wd) * p
    return p, m, v


def unscaled(g, scale):
    """The fp32 products g * float32(1 / float64(scale)), element by element; g itself without a scale."""
    if scale is None:
        return np.asarray(g, np.float32)
    return np.asarray(g, np.float32) * np.float32(1.0 / np.float64(np.float32(scale)))


def run_fp64(steps, correct_bias=True, max_norm=None, scale=None, skip=(), start=None, first=0):
    """The fixture's trajectory in fp64: per step (total_norm, coef, {name: (p, m, v, step)}) over the names that have state.
    scale: the gradients are held times ``scale`` in memory and unscaled as the kernels do.  skip: the steps (0-based) whose
    found_inf is set -- nothing changes there, the step counts included.  start: {name: (p, m, v, step)} after step ``first``."""
    P = init_params()
    state = {}
    if start is not None:
        for n, s in start.items():
            P[n] = s[0]
            state[n] = tuple(np.asarray(a, np.float64) for a in s[:3]) + (int(s[3]),)
    out = []
    for t in range(first, steps):
        grads = {}
        for n in with_grad(t):
            g = grad(n, t)
            grads[n] = unscaled(g * np.float32(scale), scale) if scale is not None else g
        total, coef = O.clip_fp64(list(grads.values()), 1.0 if max_norm is None else max_norm)
        if max_norm is None:
            coef = 1.0
        for n in grads:
            if n not in state:
                state[n] = (np.asarray(P[n], np.float64), np.zeros(P[n].shape), np.zeros(P[n].shape), 0)
            if t in skip:
                continue
            p, m, v, k = state[n]
            if p.size == 0:   # a tensor of no elements: its step is never advanced
                continue
            gi = GROUP_OF[n]
            state[n] = step_fp64(p, grads[n].astype(np.float64) * coef, m, v, k + 1, U.group_lr(gi, t), BETAS, EPS,
                                 GROUPS[gi]["weight_decay"], correct_bias) + (k + 1,)
        out.append((total, coef, dict(state)))
    return out


def layout_at(meta, run, t):
    """The layout state_dict() had after step t of a run, from adamw.json: dict(state={index: {key: type name}},
    step={index: int}, param_groups=[...]) -- a parameter has state once it has a step count."""
    lay = meta["state_dict"][run]
    return dict(state={i: lay["state_types"][i] for i in lay["step"][t]}, step=lay["step"][t],
                param_groups=[dict(pg, lr=lr) for pg, lr in zip(lay["param_groups"], lay["lr"][t])])


def bound(ref_err, scale):
    """What p, m, v are held to: 4 x the fp32 restatement's own distance from fp64, or 2 ulp of the tensor's largest magnitude."""
    return max(4 * ref_err, 2 * U.ulp32(scale))


# ------------------------------------------------------------------------------------------------------- GPU helpers
def make(max_grad_norm=None, correct_bias=True, names=NAMES, start=None):
    """({name: Parameter on the GPU}, ance_amd.optim.AdamW) on the fixture's initial values and groups."""
    import torch

    from ance_amd.optim import AdamW
    P = init_params()
    if start:
        P.update({n: s[0] for n, s in start.items()})
    params = {n: torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(P[n], np.float32)).to(DEV)) for n in names}
    groups = [dict(params=[params[n] for n in names if GROUP_OF[n] == k], lr=GROUPS[k]["lr"],
                   weight_decay=GROUPS[k]["weight_decay"]) for k in range(len(GROUPS))]
    return params, AdamW(groups, lr=1e-3, betas=BETAS, eps=EPS, correct_bias=correct_bias, max_grad_norm=max_grad_norm)


def device_grads(steps, scale=None):
    """Every step's gradients on the device up front (times ``scale``, an fp32 product), so the steps need no host copy."""
    import torch
    out = []
    for t in range(steps):
        row = {}
        for n in NAMES:
            g = grad(n, t)
            if g is not None:
                g = torch.from_numpy(g).to(DEV)
                if scale is not None:
                    g = g * torch.tensor(scale, dtype=torch.float32, device=DEV)
            row[n] = g
        out.append(row)
    return out


def set_grads(params, grads_t):
    for n in params:
        params[n].grad = None if grads_t[n] is None else grads_t[n].clone()


def set_lr(opt, t):
    for k, g in enumerate(opt.param_groups):
        g["lr"] = U.group_lr(k, t)


def set_amp(opt, grad_scale=None, found_inf=None):
    """What GradScaler.step attaches: 0-dim fp32 device tensors (None: the attribute is None)."""
    import torch
    opt.grad_scale = None if grad_scale is None else torch.full((), grad_scale, dtype=torch.float32, device=DEV)
    opt.found_inf = None if found_inf is None else torch.full((), found_inf, dtype=torch.float32, device=DEV)


def state(params, opt):
    """{name: [p, m, v, step]} as NumPy copies (p alone for a parameter without state)."""
    out = {}
    for n, p in params.items():
        st = opt.state.get(p, {})
        out[n] = [p.detach().cpu().numpy().copy()]
        if st:
            out[n] += [st["exp_avg"].cpu().numpy().copy(), st["exp_avg_sq"].cpu().numpy().copy(), st["step"].cpu().numpy().copy()]
    return out


def assert_same(a, b):
    assert a.keys() == b.keys()
    for n in a:
        assert len(a[n]) == len(b[n]), n
        for x, y in zip(a[n], b[n]):
            np.testing.assert_array_equal(x, y, err_msg=n)
