"""Objectives with gradients (ance_amd/loss.py, csrc/nll.hip, csrc/inbatch_nll.hip) and the clipped LAMB step (ance_amd/optim.py,
csrc/lamb.hip), CPU part: the fp64 restatement (tests/objective_util.py) reproduces the reference's own losses and gradients
(tests/golden/objective.*, make_golden_objective.py) -- which pins the oracle the GPU tests use -- and every refusal of the new
entry points happens on the host, before anything touches a device."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import lamb_util as U
import objective_util as O
from ance_amd import _lib

# The reference's fp32 chain against fp64, relative to the gradient's natural scale (grad_output / n) x the largest operand
# magnitude, i.e. before any cancellation: a d-term fp32 dot feeds a sigmoid / softmax (d <= 768: about sqrt(d) 2^-24 of the sum
# of |products|, a few 2^-20 of a logit of a few units) and two or three more roundings follow.  2^-16 leaves an order of
# magnitude over that and is four orders below any wrong formula, sign or index (measured on this golden: 3.5e-7 at most).
REL = 2.0 ** -16


def _golden(golden_dir):
    with open(os.path.join(golden_dir, "objective.json")) as f:
        return json.load(f), np.load(os.path.join(golden_dir, "objective.npz"))


@pytest.mark.parametrize("case", list(O.FIRSTP_CASES) + list(O.DPR_TRIPLET_CASES) + ["maxp"])
def test_triplet_oracle_reproduces_the_reference(golden_dir, case):
    j, g = _golden(golden_dir)
    q, a, b, ma, mb = O.triplet_inputs(case)
    want = O.nll_fp64(q, a, b, ma, mb)
    assert abs(j[case]["loss"] - want["loss"]) <= 4 * U.ulp32(max(1.0, want["loss"])), (j[case]["loss"], want["loss"])
    n = q.shape[0]
    worst = 0.0
    for k, operand in (("gq", max(np.abs(a).max(), np.abs(b).max())), ("ga", np.abs(q).max()), ("gb", np.abs(q).max())):
        got = g["%s.%s" % (case, k)].astype(np.float64)
        d = np.abs(got - O.recorded(want[k])).max()
        worst = max(worst, d / (operand / n))
        assert d <= REL * operand / n, (case, k, d)
        assert d <= j[case]["ref_err"][k] * (1 + 1e-12)  # the recorded distance is the maximum over the full tensor
    print(case, "worst relative distance", worst)


def test_maxp_fixture_covers_masks_and_the_tie(golden_dir):
    j, g = _golden(golden_dir)
    q, a, b, ma, mb = O.triplet_inputs("maxp")
    want = O.nll_fp64(q, a, b, ma, mb)
    assert ma[2].tolist() == [1, 0, 0, 0] and mb[3].tolist() == [1, 0, 0, 0] and ma.sum() < ma.size
    # a masked chunk never wins, and the duplicated pair is the winner of its row: the lower index
    assert all(ma[r, c] == 1 for r, c in enumerate(want["ca"])) and all(mb[r, c] == 1 for r, c in enumerate(want["cb"]))
    for name in ("a", "b"):
        r, c0, c1 = O.MAXP_DUP[name]
        assert want["c" + name][r] == c0 < c1
        # torch's max backward on the CPU puts the gradient of the tie at the lower index too: the rule is the reference's
        assert j["maxp_tie"][name]["torch_gradient_at"] == [c0]
    assert j["maxp_tie"]["rule_tested"] == "the lowest index"
    ga = g["maxp.ga"].reshape(O.MAXP_N, O.MAXP_CHUNKS, O.D)
    for r in range(O.MAXP_N):
        for c in range(O.MAXP_CHUNKS):
            assert (np.abs(ga[r, c]).max() > 0) == (c == want["ca"][r])


@pytest.mark.parametrize("case", list(O.INBATCH_CASES))
def test_inbatch_oracle_reproduces_the_reference(golden_dir, case):
    j, g = _golden(golden_dir)
    nq = O.INBATCH_CASES[case]
    q, ctx, pos = O.inbatch_inputs(nq)
    assert ctx.shape[0] == 2 * nq and pos.tolist() == [2 * i for i in range(nq)]
    want = O.inbatch_fp64(q, ctx, pos)
    assert abs(j[case]["loss"] - want["loss"]) <= 4 * U.ulp32(max(1.0, want["loss"]))
    assert j[case]["n_correct_reference"] == want["n_correct"] == j[case]["n_correct_fp64"]
    np.testing.assert_array_equal(g[case + ".correct"], want["correct"])
    assert O.inbatch_margins(q, ctx, pos).min() > 1e-3
    if nq > max(O.INBATCH_DUP_ROWS):  # the duplicate above the positive leaves it the argmax, the one below takes it
        hi, lo = O.INBATCH_DUP_ROWS
        assert want["correct"][hi] and not want["correct"][lo] and want["n_correct"] == nq - 1
    for k, operand in (("gq", 2 * np.abs(ctx).max() / nq), ("gctx", np.abs(q).max())):
        d = np.abs(g["%s.%s" % (case, k)].astype(np.float64) - O.recorded(want[k])).max()
        assert d <= REL * operand, (case, k, d, operand)


@pytest.mark.parametrize("run", list(O.CLIP_RUNS))
def test_clipped_lamb_oracle_reproduces_the_reference(golden_dir, run):
    """clip_grad_norm_ + the reference's Lamb, three steps: the bound of tests/test_lamb.py (4 ulp of each tensor's largest magnitude
    over the run, 1e-5 relative for the norms).  torch's fp32 total norm itself is 4e-6 from fp64 (a sum of 600,000 squares in
    fp32); where it clips, that relative error of coef goes once into m and twice into v (p sees m / sqrt(v), where it cancels
    up to eps), so the clipping run's bound adds 3 x that relative error of the tensor's largest magnitude."""
    j, g = _golden(golden_dir)
    traj = O.run_clipped_fp64(O.CLIP_RUNS[run])
    rel_norm = 0.0
    for t in range(O.CLIP_STEPS):
        rel_norm = max(rel_norm, abs(j["lamb_" + run]["total_norm"][t] - traj[t][0]) / traj[t][0])
        assert (traj[t][1] < 1.0) == (run == "clip")
    assert rel_norm <= 1e-5
    extra = 3 * rel_norm if run == "clip" else 0.0
    for name, *_ in U.SPEC:
        if U.grad(name, 0) is None:
            continue
        for ix, key in enumerate(("p", "m", "v")):
            want = [U.recorded(name, traj[t][2][name][ix]) for t in range(O.CLIP_STEPS)]
            scale = max(np.abs(w).max(initial=0.0) for w in want)
            tol = 4 * U.ulp32(scale) + extra * scale
            for t in range(O.CLIP_STEPS):
                got = g["lamb_%s.%s.%d.%s" % (run, name, t, key)].astype(np.float64)
                assert np.abs(got - want[t]).max(initial=0.0) <= tol, (name, t, key)
    if run == "noclip":  # never clipping: the unclipped golden's first steps, bit for bit
        g0 = np.load(os.path.join(golden_dir, "lamb.npz"))
        for t in range(O.CLIP_STEPS):
            np.testing.assert_array_equal(g["lamb_noclip.w4097.%d.p" % t], g0["lamb.w4097.%d.p" % t])


def test_max_grad_norm_is_validated_and_stays_out_of_the_state_dict():
    from ance_amd.optim import Lamb
    p = [torch.nn.Parameter(torch.zeros(3))]
    for bad in (0, 0.0, -1, -1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            Lamb(p, max_grad_norm=bad)
    assert Lamb(p).max_grad_norm is None and Lamb(p).last_grad_norm is None
    opt = Lamb(p, lr=1e-3, weight_decay=0.01, max_grad_norm=2)
    assert opt.max_grad_norm == 2.0 and opt.last_grad_norm is None
    assert opt.defaults == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01)
    sd = opt.state_dict()
    assert all("max_grad_norm" not in pg for pg in sd["param_groups"]) and sd["state"] == {}
    # no CPU fallback with clipping either
    p[0].grad = torch.ones(3)
    with pytest.raises(_lib.AnceLibraryError, match=r"param_groups\[0\]\['params'\]\[0\]"):
        opt.step()
    assert torch.equal(p[0].detach(), torch.zeros(3))


def test_cpu_tensors_are_refused_by_name():
    from ance_amd.loss import biencoder_nll_loss, nll_loss
    q, a, b = (torch.zeros(2, 128, requires_grad=True) for _ in range(3))
    with pytest.raises(_lib.AnceLibraryError, match="nll_loss: q"):
        nll_loss(q, a, b)
    with pytest.raises(_lib.AnceLibraryError, match="biencoder_nll_loss: q"):
        biencoder_nll_loss(q, a, torch.zeros(2, dtype=torch.int64))


def _refused(L, rc, name, why=None):
    assert rc == -1, (name, rc)
    msg = L.ance_last_error()
    assert name.encode() in msg and (why is None or why.encode() in msg), msg


def test_nll_backward_refusals_happen_before_any_launch():
    L = _lib.lib()
    f = ctypes.c_void_p(0x1000)

    def call(q=f, a=f, b=f, ma=None, mb=None, n=4, d=768, chunks=1, go=f, gq=f, ga=f, gb=f):
        return L.ance_nll_backward(q, a, b, ma, mb, n, d, chunks, go, gq, ga, gb, None)

    for field in ("q", "a", "b", "go", "gq", "ga", "gb"):
        _refused(L, call(**{field: None}), "ance_nll_backward")
    for kw in (dict(n=0), dict(n=-3), dict(d=0), dict(d=770), dict(d=2), dict(chunks=0), dict(chunks=4), dict(chunks=4, ma=f),
               dict(chunks=4, mb=f)):
        _refused(L, call(**kw), "ance_nll_backward")


def test_inbatch_refusals_happen_before_any_launch():
    L = _lib.lib()
    f = ctypes.c_void_p(0x1000)
    need = L.ance_inbatch_nll_workspace_bytes(128, 256, 768)
    assert need >= 2 * 128 * 256 * 4
    assert L.ance_inbatch_nll_workspace_bytes(1, 1, 128) > 0 and L.ance_inbatch_nll_workspace_bytes(1024, 2048, 1024) > 0
    outside = [(0, 2, 128), (-1, 2, 128), (1025, 2048, 128), (8, 7, 128), (8, 2049, 128), (8, 16, 124), (8, 16, 1028), (8, 16, 130),
               (8, 16, 64), (8, 16, 0)]
    for nq, nc, d in outside:
        assert L.ance_inbatch_nll_workspace_bytes(nq, nc, d) == 0, (nq, nc, d)

    def fwd(q=f, c=f, pos=f, nq=128, nc=256, d=768, mean=f, counts=f, ws=f, ws_bytes=need):
        return L.ance_inbatch_nll_forward(q, c, pos, nq, nc, d, mean, counts, ws, ws_bytes, None)

    def bwd(q=f, c=f, pos=f, nq=128, nc=256, d=768, go=f, gq=f, gc=f, ws=f, ws_bytes=need):
        return L.ance_inbatch_nll_backward(q, c, pos, nq, nc, d, go, gq, gc, ws, ws_bytes, None)

    for fn, name, own in ((fwd, "ance_inbatch_nll_forward", ("mean", "counts")), (bwd, "ance_inbatch_nll_backward", ("go", "gq", "gc"))):
        for field in ("q", "c", "pos") + own:
            _refused(L, fn(**{field: None}), name, "null pointer")
        for nq, nc, d in outside:
            _refused(L, fn(nq=nq, nc=nc, d=d), name, "shape outside")
        _refused(L, fn(ws=None), name, "workspace")
        _refused(L, fn(ws=ctypes.c_void_p(0x1008)), name, "workspace")
        _refused(L, fn(ws_bytes=need - 1), name, "workspace too small")
        _refused(L, fn(nq=256, nc=512), name, "workspace too small")


def test_clipped_step_refusals_happen_before_any_launch():
    L = _lib.lib()
    f = ctypes.c_void_p(0x1000)
    T = (_lib.AnceLambTensor * 1)()
    T[0].p = T[0].g = T[0].m = T[0].v = 0x1000
    T[0].numel, T[0].group = 8, 0
    G = (_lib.AnceLambGroup * 1)()
    G[0].lr, G[0].beta1, G[0].beta2, G[0].eps = 1e-3, 0.9, 0.999, 1e-6
    need = L.ance_lamb_clipped_workspace_bytes(1, 1, 8)
    assert need > L.ance_lamb_workspace_bytes(1, 1, 8) > 0
    assert L.ance_lamb_clipped_workspace_bytes(-1, 1, 8) == 0 and L.ance_lamb_clipped_workspace_bytes(1, 0, 8) == 0
    assert L.ance_lamb_clipped_workspace_bytes(1, 1, -1) == 0

    def call(T=T, n=1, G=G, ng=1, mx=1.0, norm=f, out=f, ws=f, ws_bytes=need):
        return L.ance_lamb_step_clipped(T, n, G, ng, 0, mx, norm, out, ws, ws_bytes, None)

    for mx in (0.0, -1.0, float("nan"), float("inf")):
        _refused(L, call(mx=mx), "ance_lamb_step_clipped", "max_grad_norm")
    _refused(L, call(norm=None), "ance_lamb_step_clipped", "d_grad_norm")
    _refused(L, call(n=-1), "ance_lamb_step_clipped", "n_tensors")
    _refused(L, call(T=None), "ance_lamb_step_clipped", "null table")
    _refused(L, call(ng=0), "ance_lamb_step_clipped", "n_groups")
    _refused(L, call(out=None), "ance_lamb_step_clipped", "d_out")
    _refused(L, call(ws=None), "ance_lamb_step_clipped", "workspace")
    _refused(L, call(ws_bytes=need - 1), "ance_lamb_step_clipped", "workspace too small")
    # the unclipped step's workspace is too small for the clipped one
    _refused(L, call(ws_bytes=L.ance_lamb_workspace_bytes(1, 1, 8)), "ance_lamb_step_clipped", "workspace too small")
    assert L.ance_lamb_step_clipped(None, 0, None, 0, 0, 1.0, None, None, None, 0, None) == 0
    # ance_lamb_step still reports under its own name
    assert L.ance_lamb_step(T, -1, G, 1, 0, f, f, need, None) == -1 and b"ance_lamb_step:" in L.ance_last_error()
