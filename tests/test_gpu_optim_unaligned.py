"""The fused optimizer steps (ance_amd.optim.Lamb, AdamW; csrc/lamb.hip, adamw.hip, multi_tensor.h) on tensors that are not 16-byte
aligned: the path on which a whole chunk goes through the scalar loop of the chunk walk, for pass 1, pass 2, the AdamW update and
the gradient-norm pass.  The parameters and gradients are contiguous views that start one element into a larger buffer:
    u3       3 elements
    u16389   16,389 elements: one full chunk on the scalar path and a 5-element second chunk
    a16389   16,389 elements, ALIGNED, in the same call: the vector path with a one-element tail across a chunk boundary
    ug1030   only the gradient is unaligned
The element arithmetic does not depend on the path, so where no sum over a tensor enters the update (AdamW without clipping,
Lamb(adam=True)) p, m, v are the bits of the same values stepped at aligned addresses.  Where one does (the trust ratio, the
clipping norm) the scalar path adds in another order: those runs are held to the fp64 restatements (tests/lamb_util.py,
adamw_util.py) by the bounds of test_gpu_lamb.py, test_gpu_lamb_clip.py and test_gpu_adamw.py, with the reference's own error taken
from its arithmetic restated in fp32 here (the goldens do not hold these tensors)."""
import functools
import math

import numpy as np
import pytest
import torch

import adamw_util as W
import lamb_util as U
import objective_util as O
from oracle.encoder_ref import det_normal

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# name, elements, group, parameter unaligned, gradient unaligned
SPEC = [("u3", 3, 0, True, True), ("u16389", 16389, 1, True, True), ("a16389", 16389, 0, False, False), ("ug1030", 1030, 1, False, True)]
NAMES = [n for n, *_ in SPEC]
GROUP_OF = {n: gi for n, _, gi, _, _ in SPEC}
STEPS = 2
MAX_NORM = 1.0   # the gradients' norm is ~1.8: clips at every step


def init(name):
    return det_normal(7, "unaligned.p." + name, (dict((n, k) for n, k, *_ in SPEC)[name],), 0.02)


def grad(name, t):
    return det_normal(100 + t, "unaligned.g." + name, (dict((n, k) for n, k, *_ in SPEC)[name],), 0.01)


def _placed(x, unaligned):
    """x on the device: a contiguous view one element (4 bytes) into a larger buffer, or a tensor of its own."""
    x = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    if not unaligned:
        t = x.to(DEV)
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.zeros(x.numel() + 8, dtype=torch.float32, device=DEV)
    buf[1:1 + x.numel()] = x
    t = buf[1:1 + x.numel()]
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def make(kind, unaligned=True, **kw):
    """({name: Parameter}, optimizer) on SPEC's values, at SPEC's addresses or (unaligned False) all aligned."""
    from ance_amd.optim import AdamW, Lamb
    params = {n: torch.nn.Parameter(_placed(init(n), unaligned and up)) for n, _, _, up, _ in SPEC}
    groups = [dict(params=[params[n] for n in NAMES if GROUP_OF[n] == k], lr=U.GROUPS[k]["lr"], weight_decay=U.GROUPS[k]["weight_decay"])
              for k in range(len(U.GROUPS))]
    cls = Lamb if kind == "lamb" else AdamW
    return params, cls(groups, lr=1e-3, betas=U.BETAS, eps=U.EPS, **kw)


def set_grads(params, t, unaligned=True, scale=None):
    for n, _, _, _, ug in SPEC:
        g = grad(n, t)
        params[n].grad = _placed(g if scale is None else g * np.float32(scale), unaligned and ug)


def state(params, opt):
    """{name: [p, m, v, step]} as NumPy copies, plus Lamb's (wn, an) and the clipping norm."""
    torch.cuda.synchronize()
    out = {}
    for n, p in params.items():
        st = opt.state[p]
        out[n] = [p.detach().cpu().numpy().copy(), st["exp_avg"].cpu().numpy().copy(), st["exp_avg_sq"].cpu().numpy().copy(),
                  np.array(float(st["step"]))]
        if "weight_norm" in st:
            out[n].append(np.array([float(st["weight_norm"]), float(st["adam_norm"])]))
    if opt.last_grad_norm is not None:
        out["grad_norm"] = [opt.last_grad_norm.cpu().numpy().copy()]
    return out


@functools.lru_cache(maxsize=None)
def run(kind, unaligned, adam, clip, scale):
    """The state after each of STEPS steps.  adam: Lamb's; scale: the gradients are held times it and grad_scale is set."""
    kw = dict(max_grad_norm=MAX_NORM if clip else None)
    if kind == "lamb":
        kw["adam"] = adam
    params, opt = make(kind, unaligned, **kw)
    out = []
    for t in range(STEPS):
        set_grads(params, t, unaligned, scale)
        if scale is not None:
            W.set_amp(opt, grad_scale=scale)
        opt.step()
        out.append(state(params, opt))
    return out


# ---------------------------------------------------------------------------------------------------- the restatements
def _clip_fp32(grads):
    """clip_grad_norm_(MAX_NORM)'s (total, coef) in fp32: the norm of the tensors' norms."""
    f = np.float32
    total = np.sqrt(sum(np.sqrt((g * g).sum(dtype=f)) ** 2 for g in grads), dtype=f)
    return total, min(f(MAX_NORM) / (total + f(1e-6)), f(1.0))


def _lamb_fp32(p, g, m, v, lr, wd, adam):
    """One step of utils/lamb.py's arithmetic, every operation rounded to fp32 as its eager tensor operations do."""
    f = np.float32
    b1, b2 = U.BETAS
    m = m * f(b1) + f(1 - b1) * g
    v = v * f(b2) + f(1 - b2) * g * g
    u = m / (np.sqrt(v) + f(U.EPS))
    if wd != 0:
        u = u + f(wd) * p
    wn = min(np.sqrt((p * p).sum(dtype=f)), f(10.0))
    an = np.sqrt((u * u).sum(dtype=f))
    tr = f(1.0) if wn == 0 or an == 0 else wn / an
    return p + (f(-lr) * (f(1.0) if adam else tr)) * u, m, v, float(wn), float(an)


def _adamw_fp32(p, g, m, v, t, lr, wd):
    """One step of transformers 2.3.0's AdamW, every tensor operation rounded to fp32; the step size a Python double."""
    f = np.float32
    b1, b2 = U.BETAS
    m = m * f(b1) + f(1 - b1) * g
    v = v * f(b2) + f(1 - b2) * g * g
    p = p + f(-lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)) * (m / (np.sqrt(v) + f(U.EPS)))
    if wd > 0:
        p = p + f(-lr * wd) * p
    return p, m, v


@functools.lru_cache(maxsize=None)
def restated(kind, adam, clip, dtype):
    """Per step (total norm, {name: (p, m, v, wn, an)}) in fp64 (lamb_util / adamw_util's restatements) or in the reference's fp32."""
    st = {n: (init(n).astype(dtype), np.zeros(init(n).shape, dtype), np.zeros(init(n).shape, dtype)) for n in NAMES}
    out = []
    for t in range(STEPS):
        grads = {n: grad(n, t).astype(dtype) for n in NAMES}
        if clip:
            total, coef = O.clip_fp64(list(grads.values()), MAX_NORM) if dtype is np.float64 else _clip_fp32(list(grads.values()))
        rec = {}
        for n in NAMES:
            p, m, v = st[n]
            g = grads[n] * coef if clip else grads[n]
            G = U.GROUPS[GROUP_OF[n]]
            if dtype is np.float64 and kind == "lamb":
                r = U.step_fp64(p, g, m, v, G["lr"], U.BETAS, U.EPS, G["weight_decay"], adam)[:5]
            elif dtype is np.float64:
                r = W.step_fp64(p, g, m, v, t + 1, G["lr"], U.BETAS, U.EPS, G["weight_decay"])
            elif kind == "lamb":
                r = _lamb_fp32(p, g, m, v, G["lr"], G["weight_decay"], adam)
            else:
                r = _adamw_fp32(p, g, m, v, t + 1, G["lr"], G["weight_decay"])
            st[n] = r[:3]
            rec[n] = r
        out.append((total if clip else None, rec))
    return out


def check_against_fp64(kind, adam, clip, pmv=True):
    """p, m, v: test_gpu_lamb.py's bound (objective_util.bound: max(4 x the reference's own max |delta| to fp64, 2 ulp of the tensor's
    largest magnitude over the steps)); wn, an: relative, max(4 x the reference's, 2^-22); the clipping norm: 1 ulp
    (test_gpu_lamb_clip.py, test_gpu_adamw.py)."""
    got = run(kind, True, adam, clip, None)
    want, ref = restated(kind, adam, clip, np.float64), restated(kind, adam, clip, np.float32)
    for n in NAMES:
        for ix, key in enumerate(("p", "m", "v")):
            if not pmv:
                break
            scale = max(np.abs(want[t][1][n][ix]).max() for t in range(STEPS))
            ref_err = max(np.abs(ref[t][1][n][ix].astype(np.float64) - want[t][1][n][ix]).max() for t in range(STEPS))
            bound = O.bound(ref_err, scale)
            for t in range(STEPS):
                d = np.abs(got[t][n][ix].astype(np.float64) - want[t][1][n][ix]).max()
                print("%s adam=%s clip=%s %s.%s step %d: %.3g (bound %.3g)" % (kind, adam, clip, n, key, t, d, bound))
                assert d <= bound, (kind, n, key, t, d, bound)
        if kind == "lamb":
            for t in range(STEPS):
                for i in range(2):
                    w = want[t][1][n][3 + i]
                    rel_ref = abs(ref[t][1][n][3 + i] - w) / abs(w)
                    rel = abs(got[t][n][4][i] - w) / abs(w)
                    print("%s adam=%s clip=%s %s norm %d step %d: %.3g (ref %.3g)" % (kind, adam, clip, n, i, t, rel, rel_ref))
                    assert rel <= max(4 * rel_ref, 2.0 ** -22), (kind, n, t, i, rel, rel_ref)
    if clip:
        for t in range(STEPS):
            assert abs(float(got[t]["grad_norm"][0]) - want[t][0]) <= U.ulp32(want[t][0]), (kind, t)


# ---------------------------------------------------------------------------------------------------------------- tests
def test_the_fixture_is_what_it_says():
    params, opt = make("adamw")
    set_grads(params, 0)
    assert [params[n].data_ptr() % 16 for n in NAMES] == [4, 4, 0, 0]
    assert [params[n].grad.data_ptr() % 16 for n in NAMES] == [4, 4, 0, 4]
    assert 16389 == 16384 + 5 and all(params[n].is_contiguous() and params[n].grad.is_contiguous() for n in NAMES)


@pytest.mark.parametrize("kind", ["adamw", "lamb"])
def test_the_element_arithmetic_does_not_depend_on_the_path(kind):
    """AdamW without clipping and Lamb(adam=True): no sum enters the update, so p, m, v are the aligned run's bits."""
    a, b = run(kind, True, True, False, None), run(kind, False, True, False, None)
    for t in range(STEPS):
        for n in NAMES:
            for x, y in zip(a[t][n][:4], b[t][n][:4]):
                np.testing.assert_array_equal(x, y, err_msg="%s step %d" % (n, t))


def test_lamb_adam_norms_against_fp64():
    check_against_fp64("lamb", adam=True, clip=False, pmv=False)


@pytest.mark.parametrize("kind,clip", [("lamb", False), ("lamb", True), ("adamw", True)])
def test_steps_that_read_a_sum_against_fp64(kind, clip):
    check_against_fp64(kind, adam=False, clip=clip)


@pytest.mark.parametrize("kind", ["adamw", "lamb"])
def test_a_power_of_two_scale_is_bit_neutral(kind):
    a, b = run(kind, True, False, True, 65536.0), run(kind, True, False, True, None)
    for t in range(STEPS):
        W.assert_same(a[t], b[t])


@pytest.mark.parametrize("kind", ["adamw", "lamb"])
def test_a_flagged_step_changes_no_bit(kind):
    params, opt = make(kind, max_grad_norm=MAX_NORM)
    set_grads(params, 0)
    opt.step()
    before = state(params, opt)
    set_grads(params, 1)
    W.set_amp(opt, found_inf=1.0)
    opt.step()
    after = state(params, opt)
    for n in NAMES:
        k = 4 if kind == "adamw" else 3   # Lamb's step is a host int that counts calls, skipped ones included
        for x, y in zip(before[n][:k], after[n][:k]):
            np.testing.assert_array_equal(x, y, err_msg=n)
    assert int(opt.skipped_steps) == 1


def test_a_refused_lamb_step_leaves_no_state():
    """The second parameter's gradient is not contiguous: the step is refused after the first parameter passed its checks, and no
    parameter has state or a changed bit."""
    from ance_amd import _lib
    from ance_amd.optim import Lamb
    a = torch.nn.Parameter(torch.from_numpy(init("u3")).to(DEV))
    b = torch.nn.Parameter(torch.from_numpy(init("ug1030")).to(DEV))
    a.grad = torch.from_numpy(grad("u3", 0)).to(DEV)
    b.grad = torch.from_numpy(np.repeat(grad("ug1030", 0), 2)).to(DEV)[::2]
    assert not b.grad.is_contiguous() and b.grad.shape == b.shape
    opt = Lamb([a, b], lr=1e-3)
    with pytest.raises(_lib.AnceLibraryError):
        opt.step()
    torch.cuda.synchronize()
    assert len(opt.state) == 0
    np.testing.assert_array_equal(a.detach().cpu().numpy(), init("u3"))
    np.testing.assert_array_equal(b.detach().cpu().numpy(), init("ug1030"))
