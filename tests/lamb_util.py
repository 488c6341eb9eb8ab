"""The LAMB step of the reference's utils/lamb.py (the optimizer drivers/run_ann.py trains with), restated in fp64 NumPy -- the
oracle of tests/test_lamb.py and tests/test_gpu_lamb.py -- and the fixture both tests and tests/golden/make_golden_lamb.py share.

One step of one tensor, with the group's hyper-parameters rounded to fp32 as the fp32 implementations use them:
    m <- b1 m + (1 - b1) g ;  v <- b2 v + (1 - b2) g^2           (no bias correction)
    u  = m / (sqrt(v) + eps), plus wd p when wd != 0 (p before the update)
    wn = min(|p|_2, 10) ;  an = |u|_2 ;  tr = 1 when wn == 0 or an == 0, else wn / an
    p <- p - lr tr u, where tr is 1 in the update when adam is set (wn, an, tr are recorded either way)
"""
import math

import numpy as np

from oracle.encoder_ref import det_normal

# name, shape, group, std of the initial values (0: zeros), std of the gradients (0: all zero, None: no gradient)
SPEC = [
    ("empty", (0,), 0, 0.5, 0.01),
    ("one", (1,), 0, 0.5, 0.01),
    ("three", (3,), 0, 0.5, 0.01),
    ("w1023", (1023,), 0, 0.02, 0.01),
    ("bias_zero", (64,), 0, 0.0, 0.01),        # wn == 0 at step 1
    ("zero_grad", (64,), 0, 0.02, 0.0),        # an == 0 every step
    ("no_grad", (5,), 0, 0.02, None),          # grad None: no state, never touched
    ("w4097", (4097,), 1, 0.02, 0.01),
    ("big", (64,), 1, 5.0, 0.01),              # |p| ~ 40: the clamp at 10 applies
    ("w768x768", (768, 768), 1, 0.02, 0.01),   # |p| ~ 15.4: clamped too
]
GROUPS = [dict(lr=1e-3, weight_decay=0.0), dict(lr=2e-3, weight_decay=0.01)]
EPS = 1e-6
BETAS = (0.9, 0.999)
STEPS = 5
# the large tensor is recorded at these flat indices only (the fixture stays small); every other tensor in full
SAMPLE_STRIDE = 1151


def lr_factor(t):
    """Learning-rate multiplier of step t (0-based): what LambdaLR(lambda t: 1 - 0.15 t) sets before step t."""
    return 1 - 0.15 * t


def group_lr(gi, t):
    return GROUPS[gi]["lr"] * lr_factor(t)


def init_params():
    out = {}
    for name, shape, _, std, _ in SPEC:
        out[name] = det_normal(7, "lamb.p." + name, shape, std) if std > 0 else np.zeros(shape, np.float32)
    return out


def grad(name, t):
    """The gradient of ``name`` at step t (0-based), or None."""
    for n, shape, _, _, gstd in SPEC:
        if n == name:
            if gstd is None:
                return None
            return det_normal(100 + t, "lamb.g." + name, shape, gstd) if gstd > 0 else np.zeros(shape, np.float32)
    raise KeyError(name)


def recorded(name, x):
    """The part of a tensor the golden keeps (flat; a copy, never a view of memory a later step changes)."""
    x = np.asarray(x).reshape(-1)
    return (x[::SAMPLE_STRIDE] if x.size > 100000 else x).copy()


def f32(x):
    return float(np.float32(x))


def step_fp64(p, g, m, v, lr, betas, eps, wd, adam):
    """One step of one tensor in fp64.  Returns (p, m, v, wn, an, tr)."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    b1, b2 = betas
    m = f32(b1) * m + f32(1 - b1) * g
    v = f32(b2) * v + f32(1 - b2) * g * g
    u = m / (np.sqrt(v) + f32(eps))
    if wd != 0:
        u = u + f32(wd) * p
    wn = min(math.sqrt(float(np.dot(p.ravel(), p.ravel()))), 10.0)
    an = math.sqrt(float(np.dot(u.ravel(), u.ravel())))
    tr = 1.0 if wn == 0 or an == 0 else wn / an
    p = p + f32(-lr) * (1.0 if adam else tr) * u
    return p, m, v, wn, an, tr


def run_fp64(steps=STEPS, adam=False, start=None, first=0):
    """The fixture's trajectory in fp64: a list over steps of {name: (p, m, v, wn, an, tr)} (names with a gradient).
    start: {name: (p, m, v)} to resume from after step ``first`` (0: from the initial values and zero state)."""
    P = init_params()
    state = {n: (P[n].astype(np.float64), np.zeros(P[n].shape), np.zeros(P[n].shape)) for n in P}
    if start is not None:
        state.update({n: tuple(np.asarray(a, np.float64) for a in s) for n, s in start.items()})
    out = []
    for t in range(first, steps):
        rec = {}
        for name, shape, gi, _, _ in SPEC:
            g = grad(name, t)
            if g is None:
                continue
            p, m, v = state[name]
            r = step_fp64(p, g, m, v, group_lr(gi, t), BETAS, EPS, GROUPS[gi]["weight_decay"], adam)
            state[name] = r[:3]
            rec[name] = r
        out.append(rec)
    return out


def ulp32(x):
    """The fp32 ulp of |x| (x >= the smallest normal)."""
    x = abs(float(x))
    if x == 0:
        return 2.0 ** -149
    return float(np.spacing(np.float32(x)))


def roberta_param_groups(kind="base"):
    """RobertaDot_NLL_LN's parameters as drivers/run_ann.py:58-78 groups them -- the embeddings, one group per layer, then the
    rest in model order -- as [(group name, [(param name, fp32 tensor, has_grad)])].  Values and shapes from
    oracle.encoder_ref.det_state_dict (the word embedding's |p| is ~124 at base size: clamped); the classifier's dense and out_proj
    (present in the model, never given a gradient) are added with zeros."""
    import torch

    from oracle.encoder_ref import det_state_dict
    hidden, inter, layers = (768, 3072, 12) if kind == "base" else (1024, 4096, 24)
    sd = det_state_dict(n_layers=layers, hidden=hidden, inter=inter)
    sd["classifier.dense.weight"], sd["classifier.dense.bias"] = torch.zeros(hidden, hidden), torch.zeros(hidden)
    sd["classifier.out_proj.weight"], sd["classifier.out_proj.bias"] = torch.zeros(2, hidden), torch.zeros(2)
    emb = [n for n in sd if n.startswith("roberta.embeddings.")]
    groups = [("embeddings", emb)]
    for i in range(layers):
        groups.append(("layer.%d" % i, [n for n in sd if n.startswith("roberta.encoder.layer.%d." % i)]))
    rest = [n for n in ("classifier.dense.weight", "classifier.dense.bias", "classifier.out_proj.weight", "classifier.out_proj.bias",
                        "embeddingHead.weight", "embeddingHead.bias", "norm.weight", "norm.bias")]
    groups.append(("rest", rest))
    assert sum(len(g) for _, g in groups) == len(sd)
    return [(gname, [(n, sd[n], not n.startswith("classifier.")) for n in names]) for gname, names in groups]
