"""Fused LAMB (ance_amd/optim.py, csrc/lamb.hip), CPU part: the fp64 restatement (tests/lamb_util.py) reproduces the reference's
own Lamb (tests/golden/lamb.*, make_golden_lamb.py) within fp32 rounding -- which pins the oracle the GPU tests use -- and every
refusal of the new C entry points happens on the host, before anything touches a device."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import lamb_util as U
from ance_amd import _lib


def _golden(golden_dir):
    with open(os.path.join(golden_dir, "lamb.json")) as f:
        return json.load(f), np.load(os.path.join(golden_dir, "lamb.npz"))


@pytest.mark.parametrize("run", ["lamb", "adam"])
def test_oracle_reproduces_the_reference(golden_dir, run):
    """The reference's fp32 chain stays within 4 ulp of each tensor's largest magnitude over the run (3.04 ulp measured) and its
    norms within 1e-5 relative (2.7e-6 measured: the 1-element tensor's m cancels at step 3)."""
    j, g = _golden(golden_dir)
    traj = U.run_fp64(adam=(run == "adam"))
    checked = 0
    for name, *_ in U.SPEC:
        if U.grad(name, 0) is None:
            assert not any(f.startswith("%s.%s." % (run, name)) and f.endswith(".norms") for f in g.files)
            for t in range(U.STEPS):
                np.testing.assert_array_equal(g["%s.%s.%d.p" % (run, name, t)], U.recorded(name, U.init_params()[name]))
            continue
        for ix, key in enumerate(("p", "m", "v")):
            if "%s.%s.0.%s" % (run, name, key) not in g.files:  # the adam run records p only (its m, v are the LAMB run's)
                continue
            want = [U.recorded(name, traj[t][name][ix]) for t in range(U.STEPS)]
            tol = 4 * U.ulp32(max(np.abs(w).max(initial=0.0) for w in want))
            for t in range(U.STEPS):
                got = g["%s.%s.%d.%s" % (run, name, t, key)].astype(np.float64)
                assert got.shape == want[t].shape
                if got.size:
                    assert np.abs(got - want[t]).max() <= tol, (name, t, key, np.abs(got - want[t]).max(), tol)
                checked += 1
        for t in range(U.STEPS):
            norms = g["%s.%s.%d.norms" % (run, name, t)].astype(np.float64)
            for got, want in zip(norms, traj[t][name][3:]):
                assert abs(got - want) <= 1e-5 * abs(want), (name, t, got, want)
    assert checked >= 5 * 8


def test_fixture_covers_the_edge_cases(golden_dir):
    j, g = _golden(golden_dir)
    assert g["lamb.bias_zero.0.norms"][0] == 0 and g["lamb.bias_zero.0.norms"][2] == 1       # wn == 0 -> tr = 1
    assert g["lamb.zero_grad.3.norms"][1] == 0 and g["lamb.zero_grad.3.norms"][2] == 1       # an == 0 -> tr = 1
    assert g["lamb.big.0.norms"][0] == 10 and g["lamb.w768x768.0.norms"][0] == 10             # the clamp
    assert g["lamb.empty.0.p"].size == 0 and g["lamb.one.0.p"].size == 1
    lay = j["state_dict_lamb"][-1]
    assert "6" not in lay["state"]                                                            # grad None: no state
    assert set(lay["state"]["0"]) == {"step", "exp_avg", "exp_avg_sq", "weight_norm", "adam_norm", "trust_ratio"}
    assert all(s == U.STEPS for s in lay["step"].values())
    assert [pg["lr"] for pg in lay["param_groups"]] == [U.group_lr(0, U.STEPS - 1), U.group_lr(1, U.STEPS - 1)]
    sz = sum(os.path.getsize(os.path.join(golden_dir, f)) for f in ("lamb.npz", "lamb.json"))
    assert sz < 512 * 1024


def test_constructor_refusals_match_the_reference():
    from ance_amd.optim import Lamb
    p = [torch.nn.Parameter(torch.zeros(3))]
    for kw, msg in ((dict(lr=-1.0), "Invalid learning rate"), (dict(eps=-1.0), "Invalid epsilon value"),
                    (dict(betas=(1.0, 0.999)), "Invalid beta parameter at index 0"),
                    (dict(betas=(0.9, 1.0)), "Invalid beta parameter at index 1")):
        with pytest.raises(ValueError, match=msg):
            Lamb(p, **kw)
    opt = Lamb(p, lr=1e-3, weight_decay=0.01, adam=True)
    assert opt.adam and opt.defaults == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01)


def test_cpu_parameters_are_refused_not_stepped_on_the_host():
    """No CPU fallback: a CPU parameter is an error naming it, and nothing is changed."""
    from ance_amd.optim import Lamb
    p = torch.nn.Parameter(torch.ones(4))
    p.grad = torch.ones(4)
    opt = Lamb([p])
    with pytest.raises(_lib.AnceLibraryError, match=r"param_groups\[0\]\['params'\]\[0\]"):
        opt.step()
    assert torch.equal(p.detach(), torch.ones(4)) and len(opt.state) == 0
    q = torch.nn.Parameter(torch.ones(2))
    q.grad = torch.sparse_coo_tensor(torch.tensor([[0]]), torch.tensor([1.0]), (2,))
    with pytest.raises(RuntimeError, match="does not support sparse gradients"):
        Lamb([q]).step()
    assert Lamb([torch.nn.Parameter(torch.ones(2))]).step(closure=lambda: 3.5) == 3.5   # no gradient: nothing to do


def _tables(n=1, numel=8, group=0, ptr=0x1000):
    T = (_lib.AnceLambTensor * max(n, 1))()
    for i in range(n):
        T[i].p = T[i].g = T[i].m = T[i].v = ptr
        T[i].numel, T[i].group = numel, group
    G = (_lib.AnceLambGroup * 1)()
    G[0].lr, G[0].beta1, G[0].beta2, G[0].eps = 1e-3, 0.9, 0.999, 1e-6
    return T, G


def test_lamb_refusals_happen_before_any_launch():
    """ance_lamb_step refuses bad tables on the host (the pointers below are never dereferenced; no device is touched)."""
    L = _lib.lib()
    fake = ctypes.c_void_p(0x1000)
    need = L.ance_lamb_workspace_bytes(1, 1, 8)
    assert need > 0
    assert L.ance_lamb_workspace_bytes(-1, 1, 8) == 0 and L.ance_lamb_workspace_bytes(1, 0, 8) == 0
    assert L.ance_lamb_workspace_bytes(1, 1, -1) == 0
    assert L.ance_lamb_workspace_bytes(201, 14, 124647168) >= L.ance_lamb_workspace_bytes(1, 1, 8)

    def call(T, n, G, ng, out=fake, ws=fake, ws_bytes=need):
        return L.ance_lamb_step(T, n, G, ng, 0, out, ws, ws_bytes, None)

    def refused(rc, why):
        assert rc == -1, rc
        msg = L.ance_last_error()
        assert b"lamb" in msg and why.encode() in msg, msg

    T, G = _tables()
    refused(call(T, -1, G, 1), "n_tensors")
    refused(call(None, 1, G, 1), "null table")
    refused(call(T, 1, None, 1), "null table")
    refused(call(T, 1, G, 0), "n_groups")
    refused(call(T, 1, G, 1, out=None), "d_out")
    refused(call(*_tables(group=1)[:1], 1, G, 1), "group index")
    refused(call(*_tables(group=-1)[:1], 1, G, 1), "group index")
    refused(call(*_tables(numel=-5)[:1], 1, G, 1), "numel")
    T0, _ = _tables()
    T0[0].m = None
    refused(call(T0, 1, G, 1), "null tensor pointer")
    refused(call(T, 1, G, 1, ws=None), "workspace")
    refused(call(T, 1, G, 1, ws=ctypes.c_void_p(0x1008)), "workspace")
    refused(call(T, 1, G, 1, ws_bytes=need - 1), "workspace too small")
    big, _ = _tables(numel=1 << 40)
    refused(call(big, 1, G, 1), "workspace too small")
    # n_tensors == 0: nothing to do, nothing enqueued
    assert L.ance_lamb_step(None, 0, None, 0, 0, None, None, 0, None) == 0
