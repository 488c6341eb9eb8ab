"""Fused LAMB (ance_amd/optim.py -> ance_lamb_step, csrc/lamb.hip) on the GPU against the fp64 restatement (tests/lamb_util.py)
and the reference's own Lamb (tests/golden/lamb.*): parity after every step, determinism, back-to-back steps, resume from the
reference's state_dict layout, LambdaLR, NaN isolation and one step at the full RoBERTa-base parameter set."""
import io
import json
import os

import numpy as np
import pytest
import torch

import lamb_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _golden(golden_dir):
    with open(os.path.join(golden_dir, "lamb.json")) as f:
        return json.load(f), np.load(os.path.join(golden_dir, "lamb.npz"))


def _make(adam=False, start=None):
    from ance_amd.optim import Lamb
    P = U.init_params()
    if start:
        P.update({n: s[0] for n, s in start.items()})
    params = {n: torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(P[n], np.float32)).to(DEV)) for n, *_ in U.SPEC}
    groups = [dict(params=[params[n] for n, _, gi, _, _ in U.SPEC if gi == k], lr=U.GROUPS[k]["lr"],
                   weight_decay=U.GROUPS[k]["weight_decay"]) for k in range(len(U.GROUPS))]
    return params, Lamb(groups, lr=1e-3, betas=U.BETAS, eps=U.EPS, adam=adam)


def _device_grads():
    """Every step's gradients on the device up front, so the steps themselves need no host copy (nor its synchronisation)."""
    return [{n: (None if U.grad(n, t) is None else torch.from_numpy(U.grad(n, t)).to(DEV)) for n, *_ in U.SPEC}
            for t in range(U.STEPS)]


def _run(params, opt, grads, steps, sync=True, set_lr=True, sched=None, record=True):
    """Steps `steps` with freshly allocated gradients each time (zero_grad sets them to None in torch >= 2)."""
    out = []
    for t in steps:
        if set_lr:
            for k, g in enumerate(opt.param_groups):
                g["lr"] = U.group_lr(k, t)
        for n, *_ in U.SPEC:
            params[n].grad = None if grads[t][n] is None else grads[t][n].clone()
        opt.step()
        if sched is not None:
            sched.step()
        if sync:
            torch.cuda.synchronize()
        if record:
            rec = {}
            for n, *_ in U.SPEC:
                st = opt.state.get(params[n], {})
                rec[n] = [params[n].detach().cpu().numpy().copy()]
                if st:
                    rec[n] += [st["exp_avg"].cpu().numpy().copy(), st["exp_avg_sq"].cpu().numpy().copy(),
                               np.array([float(st["weight_norm"]), float(st["adam_norm"]), float(st["trust_ratio"])])]
            out.append(rec)
    return out


def _ref_err(g, traj, run, name, key, ix):
    """The reference's own max |delta| to fp64 over the run (on the elements the golden keeps)."""
    k0 = "%s.%s.0.%s" % (run, name, key)
    if k0 not in g.files:  # adam run: m, v are the LAMB run's
        run = "lamb"
    return max(np.abs(g["%s.%s.%d.%s" % (run, name, t, key)].astype(np.float64) - U.recorded(name, traj[t][name][ix])).max(initial=0.0)
               for t in range(U.STEPS))


def _check_against_oracle(got, traj, g, run, steps, traj_ref=None):
    """got[j] is step steps[j]; traj: the fp64 trajectory to compare with; traj_ref: the one the golden's own error is taken
    against (the full run from step 0; default traj).  Bound: max(4 x the reference's own max |delta|, 2 ulp of the tensor's
    largest magnitude over the steps); the norms the same, relative."""
    traj_ref = traj if traj_ref is None else traj_ref
    for name, *_ in U.SPEC:
        if U.grad(name, 0) is None:
            continue
        for ix, key in enumerate(("p", "m", "v")):
            scale = max(np.abs(traj[t][name][ix]).max(initial=0.0) for t in steps)
            bound = max(4 * _ref_err(g, traj_ref, run, name, key, ix), 2 * U.ulp32(scale))
            for j, t in enumerate(steps):
                d = np.abs(got[j][name][ix].astype(np.float64) - traj[t][name][ix]).max(initial=0.0)
                assert d <= bound, (run, name, key, t, d, bound)
        for t_i, t in enumerate(steps):
            for i in range(3):
                want, want_ref = traj[t][name][3 + i], traj_ref[t][name][3 + i]
                ref = float(g["%s.%s.%d.norms" % (run, name, t)][i])
                rel_ref = abs(ref - want_ref) / abs(want_ref) if want_ref else 0.0
                rel = abs(got[t_i][name][3][i] - want) / abs(want) if want else abs(got[t_i][name][3][i])
                assert rel <= max(4 * rel_ref, 2.0 ** -22), (run, name, t, i, rel, rel_ref)


@pytest.mark.parametrize("adam", [False, True])
def test_golden_parity_every_step(golden_dir, adam):
    j, g = _golden(golden_dir)
    run = "adam" if adam else "lamb"
    params, opt = _make(adam)
    p_no_grad = params["no_grad"].detach().clone()
    got = _run(params, opt, _device_grads(), range(U.STEPS))
    _check_against_oracle(got, U.run_fp64(adam=adam), g, run, range(U.STEPS))
    assert params["no_grad"] not in opt.state and torch.equal(params["no_grad"].detach(), p_no_grad)
    # the state layout of the reference's state_dict: same indices, keys, steps, param_groups; the 0-dim tensors are tensors here
    # also where the reference stores the int 1 (tr of a tensor with wn == 0 or an == 0) -- same value, no host sync to decide
    sd = opt.state_dict()
    lay = j["state_dict_" + run][-1]
    assert sorted(str(i) for i in sd["state"]) == sorted(lay["state"])
    for i, s in sd["state"].items():
        want = lay["state"][str(i)]
        assert sorted(s) == sorted(want)
        assert type(s["step"]) is int and s["step"] == lay["step"][str(i)]
        for k in ("exp_avg", "exp_avg_sq", "weight_norm", "adam_norm", "trust_ratio"):
            assert isinstance(s[k], torch.Tensor) and s[k].dtype == torch.float32
        for k in ("weight_norm", "adam_norm", "trust_ratio"):
            assert s[k].dim() == 0 and s[k].is_cuda
        if want["trust_ratio"] == "int":
            assert float(s["trust_ratio"]) == 1.0
    assert [sorted(pg) for pg in sd["param_groups"]] == [sorted(pg) for pg in lay["param_groups"]]
    assert [pg["params"] for pg in sd["param_groups"]] == [pg["params"] for pg in lay["param_groups"]]


def test_deterministic_and_back_to_back():
    grads = _device_grads()
    a = _run(*_make(), grads, range(U.STEPS))
    b = _run(*_make(), grads, range(U.STEPS))
    params, opt = _make()
    _run(params, opt, grads, range(U.STEPS), sync=False, record=False)  # five steps, no synchronisation in between
    torch.cuda.synchronize()
    for n, *_ in U.SPEC:
        for x, y in zip(a[-1][n], b[-1][n]):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(params[n].detach().cpu().numpy(), a[-1][n][0])
        st = opt.state.get(params[n])
        if st:
            np.testing.assert_array_equal(st["exp_avg"].cpu().numpy(), a[-1][n][1])
            np.testing.assert_array_equal(st["exp_avg_sq"].cpu().numpy(), a[-1][n][2])


def test_resume_from_the_reference_state_layout(golden_dir):
    """The reference's state after step 2, in its optimizer.pt layout (CPU tensors, step ints, trust_ratio int 1 where it is
    one), loaded into a fresh optimizer, stepped to 5.  The 768 x 768 tensor is kept sampled in the golden: it resumes from
    the fp64 restatement's step-2 state rounded to fp32 instead."""
    j, g = _golden(golden_dir)
    traj = U.run_fp64()
    T0 = 2
    start, state = {}, {}
    for i, (name, *_rest) in enumerate(U.SPEC):
        if U.grad(name, 0) is None:
            continue
        shape = U.init_params()[name].shape
        if U.recorded(name, np.zeros(shape)).size == int(np.prod(shape)):
            p, m, v = (g["lamb.%s.%d.%s" % (name, T0 - 1, k)].reshape(shape) for k in ("p", "m", "v"))
        else:
            p, m, v = (traj[T0 - 1][name][k].astype(np.float32) for k in range(3))
        start[name] = (p, m, v)
        wn, an, tr = (float(x) for x in g["lamb.%s.%d.norms" % (name, T0 - 1)])
        types = j["state_dict_lamb"][T0 - 1]["state"][str(i)]
        state[i] = dict(step=T0, exp_avg=torch.from_numpy(np.array(m)), exp_avg_sq=torch.from_numpy(np.array(v)),
                        weight_norm=torch.tensor(wn), adam_norm=torch.tensor(an),
                        trust_ratio=1 if types["trust_ratio"] == "int" else torch.tensor(tr))
    pgs = [dict(pg, betas=tuple(pg["betas"])) for pg in j["state_dict_lamb"][T0 - 1]["param_groups"]]
    params, opt = _make(start=start)
    opt.load_state_dict({"state": state, "param_groups": pgs})
    assert all(opt.state[params[n]]["exp_avg"].is_cuda for n in start)
    got = _run(params, opt, _device_grads(), range(T0, U.STEPS))
    want = U.run_fp64(start=start, first=T0)
    _check_against_oracle(got, [None] * T0 + want, g, "lamb", range(T0, U.STEPS), traj_ref=traj)
    assert all(opt.state[params[n]]["step"] == U.STEPS for n in start)

    # this class's own state_dict round-trips bit for bit through torch.save / torch.load
    buf = io.BytesIO()
    torch.save(opt.state_dict(), buf)
    buf.seek(0)
    params2, opt2 = _make()
    opt2.load_state_dict(torch.load(buf, weights_only=True))
    for (a, sa), (b, sb) in zip(opt.state_dict()["state"].items(), opt2.state_dict()["state"].items()):
        assert a == b and sorted(sa) == sorted(sb)
        for k in sa:
            if isinstance(sa[k], torch.Tensor):
                assert torch.equal(sa[k].cpu(), sb[k].cpu()) and sb[k].is_cuda, (a, k)
            else:
                assert sa[k] == sb[k]


def test_lambdalr_drives_the_group_learning_rates():
    grads = _device_grads()
    want = _run(*_make(), grads, range(U.STEPS))[-1]
    params, opt = _make()
    sched = torch.optim.lr_scheduler.LambdaLR(opt, U.lr_factor)
    got = _run(params, opt, grads, range(U.STEPS), set_lr=False, sched=sched)[-1]
    for n, *_ in U.SPEC:
        for x, y in zip(got[n], want[n]):
            np.testing.assert_array_equal(x, y)


def test_nan_gradient_poisons_only_its_own_tensor():
    from ance_amd.optim import Lamb
    P = U.init_params()

    def run(with_nan):
        a = torch.nn.Parameter(torch.from_numpy(P["w4097"]).to(DEV))
        b = torch.nn.Parameter(torch.from_numpy(P["w1023"]).to(DEV))
        ga = torch.from_numpy(U.grad("w4097", 0)).to(DEV)
        if with_nan:
            ga[17] = float("nan")
        a.grad, b.grad = ga, torch.from_numpy(U.grad("w1023", 0)).to(DEV)
        opt = Lamb([a, b], lr=1e-3)
        opt.step()
        return a.detach().cpu(), b.detach().cpu(), opt.state[a], opt.state[b]

    a, b, sa, sb = run(True)
    a0, b0, _, sb0 = run(False)
    assert torch.isnan(a).all() and torch.isnan(sa["trust_ratio"]).item() and torch.isnan(sa["adam_norm"]).item()
    assert not torch.isnan(sa["weight_norm"]).item()
    assert torch.equal(b, b0) and torch.equal(sb["exp_avg"], sb0["exp_avg"]) and torch.equal(sb["trust_ratio"], sb0["trust_ratio"])


def test_full_roberta_base_step_against_fp64():
    """One step on RobertaDot_NLL_LN's 205 parameters (201 with a gradient, 124,647,168 elements) in run_ann.py's 14 groups.
    Bound: 4 ulp of each tensor's largest magnitude for p, m, v -- the fp32 chain behind an element rounds up to five times (m, v,
    sqrt, the division, the update: a zero bias's p is that whole chain) -- and 2^-22 relative for wn, an, tr (fp64 sums)."""
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
    opt = Lamb(pgs, lr=2e-5, eps=1e-8)
    assert sum(p.numel() for p in params.values() if p.grad is not None) == 124647168
    opt.step()
    torch.cuda.synchronize()
    n_checked = 0
    for gname, plist in groups:
        wd = 0.01 if gname == "rest" else 0.0
        for name, t, has_grad in plist:
            if not has_grad:
                assert params[name] not in opt.state and torch.equal(params[name].detach().cpu(), t)
                continue
            p0 = t.numpy().astype(np.float64)
            p, m, v, wn, an, tr = U.step_fp64(p0, grads[name], np.zeros_like(p0), np.zeros_like(p0), 2e-5, U.BETAS, 1e-8, wd, False)
            st = opt.state[params[name]]
            for got, want in ((params[name], p), (st["exp_avg"], m), (st["exp_avg_sq"], v)):
                d = np.abs(got.detach().cpu().numpy().astype(np.float64) - want).max()
                assert d <= 4 * U.ulp32(np.abs(want).max()), (name, d)
            for got, want in ((st["weight_norm"], wn), (st["adam_norm"], an), (st["trust_ratio"], tr)):
                assert abs(float(got) - want) <= 2.0 ** -22 * abs(want), (name, float(got), want)
            if name == "roberta.embeddings.word_embeddings.weight":
                assert float(st["weight_norm"]) == 10.0 and np.sqrt((p0 ** 2).sum()) > 100
            n_checked += 1
    assert n_checked == 201
