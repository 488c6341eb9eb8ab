"""Fused AdamW (ance_amd/optim.py AdamW, csrc/adamw.hip), CPU part: the fp64 restatement (tests/adamw_util.py) reproduces the
fp32 restatement of transformers 2.3.0's AdamW (tests/golden/adamw.*, make_golden_adamw.py) within fp32 rounding and is, where the
two coincide algebraically, torch.optim.AdamW -- which pins the oracle the GPU tests use -- and every refusal of the new C entry
point happens on the host, before anything touches a device."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch

import adamw_util as W
import lamb_util as U
from ance_amd import _lib


def _golden(golden_dir):
    with open(os.path.join(golden_dir, "adamw.json")) as f:
        return json.load(f), np.load(os.path.join(golden_dir, "adamw.npz"))


@pytest.mark.parametrize("run", list(W.RUNS))
def test_oracle_reproduces_the_golden(golden_dir, run):
    """Every recorded tensor within max(4 x the stored ref_err, 2 ulp) of the restatement run here -- so the stored ref_err is what
    this code gives -- and ref_err itself is fp32 rounding: p rounds twice a step (the update, the decay), m and v about three
    times each with the error of earlier steps damped by beta, so (steps + 1) ulp for p and 2 steps ulp for m, v of the tensor's
    largest magnitude bound them in the runs without clipping (with it, the fp32 total norm of clip_grad_norm_ enters every
    element through the clip factor, and the one-element tensor's m cancels: no bound in ulp of the result holds there)."""
    j, g = _golden(golden_dir)
    steps, correct_bias, max_norm = W.RUNS[run]
    traj = W.run_fp64(steps, correct_bias, max_norm)
    checked = 0
    for name in W.NAMES:
        for ix, key in enumerate(("p", "m", "v")):
            if key != "p" and run in W.MV_AS:
                assert "%s.%s.%d.%s" % (run, name, steps - 1, key) not in g.files
                continue
            ts = [t for t in range(steps) if name in traj[t][2]]
            if not ts:
                assert not any(f.startswith("%s.%s." % (run, name)) for f in g.files)   # grad None: no state, nothing recorded
                continue
            want = {t: U.recorded(name, traj[t][2][name][ix]) for t in ts}
            scale = max(np.abs(w).max(initial=0.0) for w in want.values())
            ref_err = max(float(g["%s.%s.%d.%s.ref_err" % (run, name, t, key)]) for t in ts)
            print("%s %s %s: ref_err %.3g = %.2f ulp" % (run, name, key, ref_err, ref_err / U.ulp32(scale)))
            if max_norm is None:
                assert ref_err <= ((steps + 1) if key == "p" else 2 * steps) * U.ulp32(scale), (name, key, ref_err)
            for t in ts:
                got = g["%s.%s.%d.%s" % (run, name, t, key)].astype(np.float64)
                assert got.shape == want[t].shape
                d = np.abs(got - want[t]).max(initial=0.0)
                assert d <= W.bound(ref_err, scale), (name, key, t, d)
                checked += 1
        if max_norm is not None:
            for t in range(steps):
                total = float(g["%s.%d.total_norm" % (run, t)])
                assert abs(total - traj[t][0]) <= 1e-5 * total, (t, total, traj[t][0])   # torch's fp32 sums: the bound of test_lamb.py's norms
    assert checked >= steps * 9   # p of nine tensors at every step, late from step 2, m and v where recorded


def test_fixture_covers_the_edge_cases(golden_dir):
    j, g = _golden(golden_dir)
    assert g["cb.empty.0.p"].size == 0 and g["cb.one.0.p"].size == 1
    assert not g["cb.zero_grad.4.m"].any() and not g["cb.zero_grad.4.v"].any()                    # zero gradients
    np.testing.assert_array_equal(g["cb.zero_grad.4.p"], U.recorded("zero_grad", W.init_params()["zero_grad"]))  # group 0: no decay
    assert not W.init_params()["bias_zero"].any() and g["cb.bias_zero.0.p"].any()
    assert "cb.late.1.p" not in g.files and "cb.late.2.p" in g.files                              # late: state from step 2
    order = j["param_order"]
    lay = [W.layout_at(j, "cb", t) for t in range(5)]
    late, no_grad, empty = (str(order.index(n)) for n in ("late", "no_grad", "empty"))
    assert late not in lay[1]["state"] and lay[2]["step"][late] == 1 and lay[4]["step"][late] == 3
    assert lay[4]["step"]["1"] == 5 and no_grad not in lay[4]["state"]
    assert lay[4]["step"][empty] == 5    # 2.3.0 counts the calls of a tensor of no elements; the fused step leaves its count at 0
    assert lay[4]["state"]["1"] == {"step": "int", "exp_avg": "Tensor", "exp_avg_sq": "Tensor"}
    assert [sorted(pg) for pg in lay[4]["param_groups"]] == [["betas", "correct_bias", "eps", "lr", "params", "weight_decay"]] * 2
    assert [pg["weight_decay"] for pg in lay[4]["param_groups"]] == [0.0, 0.01]                   # a decayed group
    assert [pg["lr"] for pg in lay[4]["param_groups"]] == [U.group_lr(0, 4), U.group_lr(1, 4)]
    # the bias correction differs between late and the rest at step 2, and the clip run clips while the other does not
    assert W.step_size(1e-3, W.BETAS, 1, True) != W.step_size(1e-3, W.BETAS, 3, True)
    clip, noclip = W.run_fp64(*W.RUNS["clip"]), W.run_fp64(*W.RUNS["noclip"])
    assert all(c[1] < 0.2 for c in clip) and all(c[1] == 1.0 for c in noclip)
    for f in ("adamw.npz", "adamw.json"):
        assert os.path.getsize(os.path.join(golden_dir, f)) < 1024 * 1024


def test_restatement_is_torch_adamw_where_the_two_coincide():
    """With eps = 0 and weight_decay = 0 the 2.3.0 step and torch.optim.AdamW are the same algebra (the eps placement and the
    decay order are all that differ).  Both in fp64 on the CPU, unrounded hyper-parameters, five steps, non-zero gradients."""
    names = ["one", "three", "w1023", "bias_zero", "w4097", "big"]
    P = W.init_params()
    params = {n: torch.nn.Parameter(torch.from_numpy(P[n].astype(np.float64))) for n in names}
    opt = torch.optim.AdamW(list(params.values()), lr=1e-3, betas=W.BETAS, eps=0.0, weight_decay=0.0)
    mine = {n: (P[n].astype(np.float64), np.zeros(P[n].shape), np.zeros(P[n].shape)) for n in names}
    for t in range(5):
        lr = U.group_lr(0, t)
        opt.param_groups[0]["lr"] = lr
        for n in names:
            g = W.grad(n, t).astype(np.float64)
            assert t > 0 or np.all(g != 0)   # v > 0 from the first step on: no 0 / 0 with eps = 0
            params[n].grad = torch.from_numpy(g.copy())
            mine[n] = W.step_fp64(*mine[n][:1], g, *mine[n][1:], t + 1, lr, W.BETAS, 0.0, 0.0, True, rnd=float)
        opt.step()
        for n in names:
            st = opt.state[params[n]]
            for got, want in zip(mine[n], (params[n].detach(), st["exp_avg"], st["exp_avg_sq"])):
                np.testing.assert_allclose(got, want.numpy(), rtol=1e-12, atol=0.0, err_msg="%s step %d" % (n, t))


def test_skipped_steps_of_the_restatement_leave_the_counts():
    """A skipped step changes nothing, its count included: the trajectory after it is the one in which the call never happened but
    for the gradients and learning rates (those of the later step)."""
    sk = W.run_fp64(2, skip=(0,))
    P = W.init_params()
    for n, (p, m, v, k) in sk[0][2].items():
        np.testing.assert_array_equal(p, P[n].astype(np.float64))
        assert k == 0 and not m.any() and not v.any()
    assert all(k == (0 if P[n].size == 0 else 1) for n, (_, _, _, k) in sk[1][2].items())
    pow2 = W.run_fp64(3, max_norm=1.0, scale=65536.0)
    for a, b in zip(pow2, W.run_fp64(3, max_norm=1.0)):
        assert a[0] == b[0] and a[1] == b[1]
        for n in b[2]:
            for x, y in zip(a[2][n], b[2][n]):
                np.testing.assert_array_equal(x, y, err_msg=n)


def test_constructor_as_transformers_2_3_0():
    from ance_amd.optim import AdamW
    p = [torch.nn.Parameter(torch.zeros(3))]
    for kw, msg in ((dict(lr=-1.0), "Invalid learning rate"), (dict(eps=-1.0), "Invalid epsilon value"),
                    (dict(betas=(1.0, 0.999)), "Invalid beta parameter"), (dict(betas=(-0.1, 0.999)), "Invalid beta parameter"),
                    (dict(betas=(0.9, 1.0)), "Invalid beta parameter"), (dict(max_grad_norm=0.0), "Invalid max_grad_norm"),
                    (dict(max_grad_norm=float("inf")), "Invalid max_grad_norm"), (dict(max_grad_norm="x"), "Invalid max_grad_norm")):
        with pytest.raises(ValueError, match=msg):
            AdamW(p, **kw)
    opt = AdamW(p)
    assert opt.defaults == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, correct_bias=True)
    assert opt.max_grad_norm is None and opt.last_grad_norm is None and opt.skipped_steps is None
    opt = AdamW(p, lr=2e-5, eps=1e-8, weight_decay=0.01, correct_bias=False, max_grad_norm=1)
    assert opt.max_grad_norm == 1.0 and opt.param_groups[0]["correct_bias"] is False
    # GradScaler's contract for fused optimizers, and a file layout that holds nothing but 2.3.0's entries
    assert AdamW._step_supports_amp_scaling is True
    assert list(inspect.signature(AdamW.step).parameters) == ["self", "closure"]
    assert "grad_scaler" not in inspect.signature(opt.step).parameters
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"}
    assert sorted(sd["param_groups"][0]) == ["betas", "correct_bias", "eps", "lr", "params", "weight_decay"]


def test_load_state_dict_takes_the_reference_layout_and_state_dict_returns_it():
    """step: a Python int in the file, an fp32 0-dim tensor on the parameter's device in the live state (a CPU parameter here: the
    conversion is host code; the step itself refuses it)."""
    from ance_amd.optim import AdamW
    p = torch.nn.Parameter(torch.zeros(3))
    opt = AdamW([p])
    ref = {"state": {0: {"step": 7, "exp_avg": torch.ones(3), "exp_avg_sq": torch.full((3,), 2.0)}},
           "param_groups": opt.state_dict()["param_groups"]}
    opt.load_state_dict(ref)
    st = opt.state[p]
    assert isinstance(st["step"], torch.Tensor) and st["step"].dtype == torch.float32 and st["step"].dim() == 0 and float(st["step"]) == 7
    sd = opt.state_dict()
    assert type(sd["state"][0]["step"]) is int and sd["state"][0]["step"] == 7
    assert isinstance(opt.state[p]["step"], torch.Tensor)          # the live state keeps its tensor
    assert torch.equal(sd["state"][0]["exp_avg"], torch.ones(3))
    opt2 = AdamW([torch.nn.Parameter(torch.zeros(3))])
    opt2.load_state_dict(sd)                                       # and its own file loads again
    assert float(opt2.state[opt2.param_groups[0]["params"][0]]["step"]) == 7


def test_cpu_parameters_are_refused_not_stepped_on_the_host():
    """No CPU fallback: a CPU parameter is an error naming it, and nothing is changed."""
    from ance_amd.optim import AdamW
    p = torch.nn.Parameter(torch.ones(4))
    p.grad = torch.ones(4)
    opt = AdamW([p])
    with pytest.raises(_lib.AnceLibraryError, match=r"AdamW: param_groups\[0\]\['params'\]\[0\]"):
        opt.step()
    assert torch.equal(p.detach(), torch.ones(4)) and len(opt.state) == 0
    q = torch.nn.Parameter(torch.ones(2))
    q.grad = torch.sparse_coo_tensor(torch.tensor([[0]]), torch.tensor([1.0]), (2,))
    with pytest.raises(RuntimeError, match="does not support sparse gradients"):
        AdamW([q]).step()
    assert AdamW([torch.nn.Parameter(torch.ones(2))]).step(closure=lambda: 3.5) == 3.5   # no gradient: nothing to do


def test_workspace_bytes_is_pure_and_larger_with_clip():
    L = _lib.lib()
    for args in ((1, 1, 8), (10, 2, 600000), (201, 14, 124647168), (393, 26, 355098880), (0, 1, 0)):
        plain, clip = L.ance_adamw_workspace_bytes(*args, 0), L.ance_adamw_workspace_bytes(*args, 1)
        assert plain == L.ance_adamw_workspace_bytes(*args, 0) and clip == L.ance_adamw_workspace_bytes(*args, 1)
        assert clip > plain and (plain > 0 or args[0] == 0)
    for args in ((-1, 1, 8), (1, 0, 8), (1, 1, -1), (1, 1, 1 << 50)):
        assert L.ance_adamw_workspace_bytes(*args, 0) == 0 and L.ance_adamw_workspace_bytes(*args, 1) == 0


def _tables(n=1, numel=8, group=0, ptr=0x1000):
    T = (_lib.AnceAdamwTensor * max(n, 1))()
    for i in range(n):
        T[i].p = T[i].g = T[i].m = T[i].v = T[i].step = ptr
        T[i].numel, T[i].group = numel, group
    G = (_lib.AnceLambGroup * 1)()
    G[0].lr, G[0].beta1, G[0].beta2, G[0].eps = 1e-3, 0.9, 0.999, 1e-6
    return T, G


def test_adamw_refusals_happen_before_any_launch():
    """ance_adamw_step refuses on the host (the pointers below are fake and never dereferenced; no device is touched): everything
    ance_lamb_step_amp refuses, and a null step of a tensor with elements."""
    L = _lib.lib()
    fake = ctypes.c_void_p(0x1000)
    need = L.ance_adamw_workspace_bytes(1, 1, 8, 1)

    def call(T, n, G, ng, mx=1.0, norm=fake, ws=fake, ws_bytes=need, scale=fake, inf=fake, skipped=fake, cb=1):
        return L.ance_adamw_step(T, n, G, ng, cb, mx, scale, inf, norm, skipped, ws, ws_bytes, None)

    def refused(rc, why):
        assert rc == -1, rc
        msg = L.ance_last_error()
        assert b"ance_adamw_step" in msg and why.encode() in msg, msg

    T, G = _tables()
    for mx in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        refused(call(T, 1, G, 1, mx=mx), "max_grad_norm")
    refused(call(T, 1, G, 1, norm=None), "d_grad_norm")
    for amp in (dict(), dict(scale=None, inf=None, skipped=None)):   # with and without the optional pointers
        for mx in (0.0, 1.0):
            for cb in (0, 1):
                kw = dict(amp, mx=mx, cb=cb)
                refused(call(T, -1, G, 1, **kw), "n_tensors")
                refused(call(None, 1, G, 1, **kw), "null table")
                refused(call(T, 1, None, 1, **kw), "null table")
                refused(call(T, 1, G, 0, **kw), "n_groups")
                refused(call(*_tables(group=1)[:1], 1, G, 1, **kw), "group index")
                refused(call(*_tables(group=-1)[:1], 1, G, 1, **kw), "group index")
                refused(call(*_tables(numel=-5)[:1], 1, G, 1, **kw), "numel")
                for field in ("p", "g", "m", "v"):
                    T0, _ = _tables()
                    setattr(T0[0], field, None)
                    refused(call(T0, 1, G, 1, **kw), "null tensor pointer")
                T0, _ = _tables()
                T0[0].step = None
                refused(call(T0, 1, G, 1, **kw), "null step")
                refused(call(T, 1, G, 1, ws=None, **kw), "workspace")
                refused(call(T, 1, G, 1, ws=ctypes.c_void_p(0x1008), **kw), "workspace")
                refused(call(*_tables(numel=1 << 40)[:1], 1, G, 1, **kw), "workspace too small")
    refused(call(T, 1, G, 1, mx=0.0, norm=None, ws_bytes=L.ance_adamw_workspace_bytes(1, 1, 8, 0) - 1), "workspace too small")
    refused(call(T, 1, G, 1, mx=1.0, ws_bytes=need - 1), "workspace too small")
    # n_tensors == 0: nothing to do, nothing enqueued
    assert L.ance_adamw_step(None, 0, None, 0, 1, 1.0, None, None, None, None, None, 0, None) == 0
