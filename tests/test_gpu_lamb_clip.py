"""Gradient clipping fused into the LAMB step (ance_amd.optim.Lamb(max_grad_norm=...) -> ance_lamb_step_clipped, csrc/lamb.hip) on
the GPU: against the unclipped step, against "scale the gradients with torch, then the plain fused step", against the fp64
restatement (tests/objective_util.py) and against clip_grad_norm_ + the reference's own Lamb (tests/golden/objective.*)."""
import json
import os

import numpy as np
import pytest
import torch

import lamb_util as U
import objective_util as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = [n for n, *_ in U.SPEC]
WITH_GRAD = [n for n in NAMES if U.grad(n, 0) is not None]


def _make(max_grad_norm=None, names=NAMES):
    from ance_amd.optim import Lamb
    P = U.init_params()
    params = {n: torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(P[n], np.float32)).to(DEV)) for n in names}
    groups = [dict(params=[params[n] for n, _, gi, _, _ in U.SPEC if gi == k and n in params], lr=U.GROUPS[k]["lr"],
                   weight_decay=U.GROUPS[k]["weight_decay"]) for k in range(len(U.GROUPS))]
    return params, Lamb(groups, lr=1e-3, betas=U.BETAS, eps=U.EPS, max_grad_norm=max_grad_norm)


def _set_grads(params, t, scale=None):
    for n in params:
        g = U.grad(n, t)
        if g is None:
            params[n].grad = None
        else:
            g = torch.from_numpy(g).to(DEV)
            params[n].grad = g if scale is None else g * scale  # an fp32 product, element by element


def _set_lr(opt, t):
    for k, g in enumerate(opt.param_groups):
        g["lr"] = U.group_lr(k, t)


def _state(params, opt):
    out = {}
    for n, p in params.items():
        st = opt.state.get(p, {})
        out[n] = [p.detach().cpu().numpy().copy()]
        if st:
            out[n] += [st["exp_avg"].cpu().numpy().copy(), st["exp_avg_sq"].cpu().numpy().copy(),
                       np.array([float(st["weight_norm"]), float(st["adam_norm"]), float(st["trust_ratio"])], np.float32)]
    return out


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for n in a:
        assert len(a[n]) == len(b[n]), n
        for x, y in zip(a[n], b[n]):
            np.testing.assert_array_equal(x, y, err_msg=n)


def test_a_norm_below_max_grad_norm_changes_no_bit():
    pc, oc = _make(max_grad_norm=1000.0)
    pu, ou = _make()
    for t in range(3):
        for params, opt in ((pc, oc), (pu, ou)):
            _set_lr(opt, t)
            _set_grads(params, t)
            opt.step()
        _assert_same(_state(pc, oc), _state(pu, ou))
    assert ou.last_grad_norm is None and oc.last_grad_norm.dim() == 0 and oc.last_grad_norm.is_cuda
    assert 7.0 < float(oc.last_grad_norm) < 8.0


def test_clipping_equals_scaled_gradients_then_the_plain_step_and_the_norm_is_right():
    """array_equal to: multiply every gradient by the coef the step reported (max_grad_norm / (last_grad_norm + 1e-6), fp32) with
    torch, then the plain fused step.  last_grad_norm within 1 ulp and coef within 2 ulp of the fp64 restatement: one rounding of
    an fp64 sum, then one fp32 add and one fp32 divide."""
    mx = O.CLIP_RUNS["clip"]
    pc, oc = _make(max_grad_norm=mx)
    pu, ou = _make()
    for t in range(3):
        _set_lr(oc, t)
        _set_grads(pc, t)
        before = {n: pc[n].grad.clone() for n in WITH_GRAD}
        oc.step()
        norm = oc.last_grad_norm
        coef = torch.tensor(mx, dtype=torch.float32, device=DEV) / (norm + torch.tensor(1e-6, dtype=torch.float32, device=DEV))
        assert coef.dtype == torch.float32 and float(coef) < 1.0
        want_norm, want_coef = O.clip_fp64([U.grad(n, t) for n in WITH_GRAD], mx)
        print("step %d: norm %.9g (fp64 %.12g)  coef %.9g (fp64 %.12g)" % (t, float(norm), want_norm, float(coef), want_coef))
        assert abs(float(norm) - want_norm) <= U.ulp32(want_norm)
        assert abs(float(coef) - want_coef) <= 2 * U.ulp32(want_coef)
        for n in WITH_GRAD:  # p.grad keeps its bits
            assert torch.equal(pc[n].grad, before[n]), n
        _set_lr(ou, t)
        _set_grads(pu, t, scale=coef)
        ou.step()
        _assert_same(_state(pc, oc), _state(pu, ou))


@pytest.mark.parametrize("run", list(O.CLIP_RUNS))
def test_golden_trajectory_of_three_steps(golden_dir, run):
    """clip_grad_norm_ + the reference's Lamb.  Bound as tests/test_gpu_lamb.py: max(4 x the reference's own max |delta| to fp64
    over the run, 2 ulp of the tensor's largest magnitude); the norms the same, relative."""
    with open(os.path.join(golden_dir, "objective.json")) as f:
        j = json.load(f)
    g = np.load(os.path.join(golden_dir, "objective.npz"))
    mx = O.CLIP_RUNS[run]
    traj = O.run_clipped_fp64(mx)
    params, opt = _make(max_grad_norm=mx)
    got = []
    for t in range(O.CLIP_STEPS):
        _set_lr(opt, t)
        _set_grads(params, t)
        opt.step()
        got.append(_state(params, opt))
        ref_rel = abs(j["lamb_" + run]["total_norm"][t] - traj[t][0]) / traj[t][0]
        assert abs(float(opt.last_grad_norm) - traj[t][0]) / traj[t][0] <= max(4 * ref_rel, 2.0 ** -22)
    for name in WITH_GRAD:
        for ix, key in enumerate(("p", "m", "v")):
            scale = max(np.abs(traj[t][2][name][ix]).max(initial=0.0) for t in range(O.CLIP_STEPS))
            ref_err = max(np.abs(g["lamb_%s.%s.%d.%s" % (run, name, t, key)].astype(np.float64)
                                 - U.recorded(name, traj[t][2][name][ix])).max(initial=0.0) for t in range(O.CLIP_STEPS))
            bound = O.bound(ref_err, scale)
            for t in range(O.CLIP_STEPS):
                d = np.abs(got[t][name][ix].astype(np.float64) - traj[t][2][name][ix]).max(initial=0.0)
                assert d <= bound, (run, name, key, t, d, bound)
        for t in range(O.CLIP_STEPS):
            for i in range(3):
                want = traj[t][2][name][3 + i]
                ref = float(g["lamb_%s.%s.%d.norms" % (run, name, t)][i])
                rel_ref = abs(ref - want) / abs(want) if want else 0.0
                rel = abs(got[t][name][3][i] - want) / abs(want) if want else abs(got[t][name][3][i])
                assert rel <= max(4 * rel_ref, 2.0 ** -22), (run, name, t, i, rel, rel_ref)


def test_nan_in_one_gradient_poisons_every_stepped_tensor():
    params, opt = _make(max_grad_norm=1.0, names=["w4097", "w1023", "no_grad"])
    _set_grads(params, 0)
    params["w4097"].grad[17] = float("nan")
    keep = params["no_grad"].detach().clone()
    opt.step()
    assert torch.isnan(opt.last_grad_norm).item()
    for n in ("w4097", "w1023"):
        assert torch.isnan(params[n]).all(), n
        assert torch.isnan(opt.state[params[n]]["exp_avg"]).all()
    assert torch.equal(params["no_grad"].detach(), keep) and params["no_grad"] not in opt.state


def test_parameters_without_gradient_stay_out_and_two_groups_share_one_norm():
    params, opt = _make(max_grad_norm=1.0)
    assert opt.param_groups[0]["lr"] != opt.param_groups[1]["lr"]
    _set_grads(params, 0)
    assert params["no_grad"].grad is None
    keep = params["no_grad"].detach().clone()
    opt.step()
    # one norm over both groups' gradients (a per-group norm would be smaller than either of these)
    want, _ = O.clip_fp64([U.grad(n, 0) for n in WITH_GRAD], 1.0)
    per_group = [O.clip_fp64([U.grad(n, 0) for n, _, gi, _, _ in U.SPEC if gi == k and n in WITH_GRAD], 1.0)[0] for k in (0, 1)]
    assert abs(float(opt.last_grad_norm) - want) <= U.ulp32(want) and all(abs(pg - want) > 100 * U.ulp32(want) for pg in per_group)
    assert torch.equal(params["no_grad"].detach(), keep) and params["no_grad"] not in opt.state
    # a parameter that has no gradient but a huge value does not enter the norm
    params2, opt2 = _make(max_grad_norm=1.0)
    with torch.no_grad():
        params2["no_grad"].fill_(1e6)
    _set_grads(params2, 0)
    opt2.step()
    assert torch.equal(opt2.last_grad_norm, opt.last_grad_norm)
    for n in WITH_GRAD:
        assert torch.equal(params2[n], params[n]), n


def test_deterministic():
    runs = []
    for _ in range(2):
        params, opt = _make(max_grad_norm=1.0)
        for t in range(3):
            _set_lr(opt, t)
            _set_grads(params, t)
            opt.step()
        runs.append((_state(params, opt), opt.last_grad_norm.cpu().numpy()))
    _assert_same(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])


def test_full_roberta_base_clipped_step_against_fp64():
    """One clipped step on RobertaDot_NLL_LN's 205 parameters (201 with a gradient, 124,647,168 elements).  Bound as
    test_full_roberta_base_step_against_fp64: 4 ulp of each tensor's largest magnitude for p, m, v (the chain rounds once more,
    g coef, and the first step's m, v are single products of it: still within the five roundings that bound counts for p) and 2^-22
    relative for wn, an, tr; the total norm within 1 ulp."""
    from ance_amd.optim import Lamb
    from oracle.encoder_ref import det_normal
    groups = U.roberta_param_groups("base")
    params, pgs, grads = {}, [], {}
    for gname, plist in groups:
        ps = []
        for name, t, has_grad in plist:
            params[name] = torch.nn.Parameter(t.to(DEV))
            if has_grad:
                grads[name] = det_normal(5, "grad." + name, tuple(t.shape), 1e-3)
                params[name].grad = torch.from_numpy(grads[name]).to(DEV)
            ps.append(params[name])
        pgs.append(dict(params=ps, weight_decay=0.01 if gname == "rest" else 0.0))
    opt = Lamb(pgs, lr=2e-5, eps=1e-8, max_grad_norm=1.0)
    opt.step()
    torch.cuda.synchronize()
    total, coef = O.clip_fp64(list(grads.values()), 1.0)
    assert coef < 1.0  # 124.6 M elements of std 1e-3: the norm is ~11.2
    print("total norm %.9g (fp64 %.12g)" % (float(opt.last_grad_norm), total))
    assert abs(float(opt.last_grad_norm) - total) <= U.ulp32(total)
    n_checked = 0
    for gname, plist in groups:
        wd = 0.01 if gname == "rest" else 0.0
        for name, t, has_grad in plist:
            if not has_grad:
                assert params[name] not in opt.state and torch.equal(params[name].detach().cpu(), t)
                continue
            p0 = t.numpy().astype(np.float64)
            p, m, v, wn, an, tr = U.step_fp64(p0, grads[name].astype(np.float64) * coef, np.zeros_like(p0), np.zeros_like(p0), 2e-5,
                                              U.BETAS, 1e-8, wd, False)
            st = opt.state[params[name]]
            for got, want in ((params[name], p), (st["exp_avg"], m), (st["exp_avg_sq"], v)):
                d = np.abs(got.detach().cpu().numpy().astype(np.float64) - want).max()
                assert d <= 4 * U.ulp32(np.abs(want).max()), (name, d)
            for got, want in ((st["weight_norm"], wn), (st["adam_norm"], an), (st["trust_ratio"], tr)):
                assert abs(float(got) - want) <= 2.0 ** -22 * abs(want), (name, float(got), want)
            n_checked += 1
    assert n_checked == 201
