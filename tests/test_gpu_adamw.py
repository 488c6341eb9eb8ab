"""Fused AdamW on the GPU (ance_amd.optim.AdamW -> ance_adamw_step, csrc/adamw.hip) against the fp64 restatement of transformers
2.3.0's AdamW (tests/adamw_util.py) and its fp32 restatement (tests/golden/adamw.*): parity after every step of four trajectories,
then the properties that hold bit for bit -- determinism, a clip that does not clip, loss scaling, the skip on the device that
leaves the step counts -- then NaN gradients, a real GradScaler, resume in both directions and the refusals.  Fixture:
adamw_util.SPEC (sizes 0, 1, 3, 1023, 4097 and a 36-chunk tensor, two groups, a None gradient, a tensor whose gradients start late)."""
import functools
import io
import json
import os

import numpy as np
import pytest
import torch

import adamw_util as W
import lamb_util as U
from ance_amd import _lib

pytestmark = pytest.mark.gpu

DEV = W.DEV
S16 = 65536.0
CLIPS = [1.0, None]   # the fixture's gradient norm is ~7.7: 1.0 clips at every step


def _golden(golden_dir):
    with open(os.path.join(golden_dir, "adamw.json")) as f:
        return json.load(f), np.load(os.path.join(golden_dir, "adamw.npz"))


@functools.lru_cache(maxsize=None)
def _grads(scale=None):
    return W.device_grads(5, scale)


def _step(params, opt, t, scale=None, set_lr=True):
    if set_lr:
        W.set_lr(opt, t)
    W.set_grads(params, _grads(scale)[t])
    opt.step()


@functools.lru_cache(maxsize=None)
def _plain(max_grad_norm, steps=(0, 1, 2), correct_bias=True):
    """The step with neither grad_scale nor found_inf at the given steps' gradients and learning rates: per step (state,
    last_grad_norm bits or None).  Computed once, never changed."""
    params, opt = W.make(max_grad_norm, correct_bias)
    out = []
    for t in steps:
        _step(params, opt, t)
        out.append((W.state(params, opt), None if opt.last_grad_norm is None else opt.last_grad_norm.cpu().numpy().copy()))
    assert opt.skipped_steps is None
    return out


def _norm_bits(opt):
    return None if opt.last_grad_norm is None else opt.last_grad_norm.cpu().numpy()


def _ref_err(g, run, name, key, steps):
    if key != "p":
        run = W.MV_AS.get(run, run)
    return max(float(g["%s.%s.%d.%s.ref_err" % (run, name, t, key)]) for t in range(steps)
               if "%s.%s.%d.%s.ref_err" % (run, name, t, key) in g.files)


def _check_against_oracle(got, traj, g, run, steps, ref_steps):
    """got[j]: adamw_util.state after step steps[j]; traj[t]: the fp64 trajectory.  Bound: max(4 x the golden's own max |delta| to
    fp64 over the run, 2 ulp of the tensor's largest magnitude over the steps)."""
    checked = 0
    for name in W.NAMES:
        ts = [t for t in steps if name in traj[t][2]]
        for j, t in enumerate(steps):
            assert (len(got[j][name]) == 4) == (t in ts), (name, t)   # state exactly where the restatement has it
        if not ts:
            continue
        for ix, key in enumerate(("p", "m", "v")):
            scale = max(np.abs(traj[t][2][name][ix]).max(initial=0.0) for t in ts)
            bound = W.bound(_ref_err(g, run, name, key, ref_steps), scale)
            for j, t in enumerate(steps):
                if t not in ts:
                    continue
                d = np.abs(got[j][name][ix].astype(np.float64) - traj[t][2][name][ix]).max(initial=0.0)
                print("%s %s.%s step %d: %.3g (bound %.3g)" % (run, name, key, t, d, bound))
                assert d <= bound, (run, name, key, t, d, bound)
                checked += 1
        for j, t in enumerate(steps):
            if t in ts:
                assert got[j][name][3] == traj[t][2][name][3], (name, t)   # the device step count
    return checked


@pytest.mark.parametrize("run", list(W.RUNS))
def test_golden_parity_every_step_under_lambdalr(golden_dir, run):
    """1, 2: every step of the trajectory within the bound, LambdaLR driving the group learning rates; late gets state at step 2
    with step == 1; the None-gradient parameter has no state and its bits; the tensor of no elements is accepted."""
    j, g = _golden(golden_dir)
    steps, correct_bias, max_norm = W.RUNS[run]
    params, opt = W.make(max_norm, correct_bias)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, U.lr_factor)
    p_no_grad = params["no_grad"].detach().clone()
    got = []
    for t in range(steps):
        _step(params, opt, t, set_lr=False)
        sched.step()
        got.append(W.state(params, opt))
        if t == W.LATE_FROM - 1:
            assert params["late"] not in opt.state
        if t == W.LATE_FROM:
            st = opt.state[params["late"]]["step"]
            assert st.is_cuda and st.dtype == torch.float32 and st.dim() == 0 and float(st) == 1.0
    traj = W.run_fp64(steps, correct_bias, max_norm)
    assert _check_against_oracle(got, traj, g, run, range(steps), steps) >= steps * 9 * 3
    assert params["no_grad"] not in opt.state and torch.equal(params["no_grad"].detach(), p_no_grad)
    assert params["empty"] in opt.state and opt.state[params["empty"]]["exp_avg"].numel() == 0
    if max_norm is not None:
        want = traj[-1][0]
        assert abs(float(opt.last_grad_norm) - want) <= U.ulp32(want)
    else:
        assert opt.last_grad_norm is None


def test_deterministic_and_back_to_back():
    """3: two runs are bit-identical; two steps enqueued without a synchronise in between equal two synchronised steps."""
    a, b = _plain(1.0, steps=(0, 1)), None
    params, opt = W.make(1.0)
    for t in (0, 1):
        _step(params, opt, t)
        torch.cuda.synchronize()
    b = W.state(params, opt)
    W.assert_same(a[1][0], b)
    params, opt = W.make(1.0)
    grads = _grads()
    torch.cuda.synchronize()
    for t in (0, 1):                     # nothing between the two steps reads the device
        W.set_lr(opt, t)
        W.set_grads(params, grads[t])
        opt.step()
    torch.cuda.synchronize()
    W.assert_same(a[1][0], W.state(params, opt))


def test_a_clip_that_does_not_clip_gives_the_plain_bits():
    """4: a total norm below max_grad_norm: coef == 1 and the plain step's bits; last_grad_norm is the fp64 norm to 1 ulp (one
    rounding of an fp64 sum)."""
    params, opt = W.make(1000.0)
    traj = W.run_fp64(3, max_norm=1000.0)
    for t, (want, _) in enumerate(_plain(None)):
        _step(params, opt, t)
        W.assert_same(W.state(params, opt), want)
        print("step %d: norm %.9g (fp64 %.12g)" % (t, float(opt.last_grad_norm), traj[t][0]))
        assert abs(float(opt.last_grad_norm) - traj[t][0]) <= U.ulp32(traj[t][0])
        assert 7.0 < traj[t][0] < 8.0


@pytest.mark.parametrize("mx", CLIPS)
def test_power_of_two_scale_is_bit_neutral(mx):
    """5: grad_scale = 65536 on gradients times 65536: the plain step's bits, and p.grad keeps its scaled bits."""
    params, opt = W.make(mx)
    W.set_amp(opt, grad_scale=S16, found_inf=0.0)
    for t, (want, want_norm) in enumerate(_plain(mx)):
        _step(params, opt, t, scale=S16)
        W.assert_same(W.state(params, opt), want)
        for n in W.with_grad(t):
            assert torch.equal(params[n].grad, _grads(S16)[t][n]), n
            assert torch.equal(params[n].grad, _grads()[t][n] * S16), n
        if mx is None:
            assert opt.last_grad_norm is None
        else:
            np.testing.assert_array_equal(_norm_bits(opt), want_norm)
    assert int(opt.skipped_steps) == 0 and opt.skipped_steps.dtype == torch.int64 and opt.skipped_steps.dim() == 0


@pytest.mark.parametrize("mx", CLIPS)
def test_general_scale_equals_torch_unscaling_then_the_plain_step(mx):
    """6: grad_scale = 3000: equal, bit for bit, to multiplying every gradient by float32(1 / float64(3000)) with torch and then the
    plain step."""
    scale = 3000.0
    inv_np = np.float32(1.0 / np.float64(np.float32(scale)))
    inv = torch.tensor(float(inv_np), dtype=torch.float32, device=DEV)
    assert inv.cpu().numpy() == inv_np and float(inv) * scale != 1.0   # not a power of two: the product rounds
    pa, oa = W.make(mx)
    pr, orf = W.make(mx)
    W.set_amp(oa, grad_scale=scale, found_inf=0.0)
    for t in range(3):
        for params, opt in ((pa, oa), (pr, orf)):
            W.set_lr(opt, t)
            W.set_grads(params, _grads(scale)[t])
        for n in W.with_grad(t):
            pr[n].grad = pr[n].grad * inv
        oa.step()
        orf.step()
        W.assert_same(W.state(pa, oa), W.state(pr, orf))
        for n in W.with_grad(t):
            assert torch.equal(pa[n].grad, _grads(scale)[t][n]), n
        if mx is not None:
            assert torch.equal(oa.last_grad_norm, orf.last_grad_norm)
            want = W.run_fp64(t + 1, max_norm=mx, scale=scale)[t][0]
            assert abs(float(oa.last_grad_norm) - want) <= U.ulp32(want)


@pytest.mark.parametrize("flag", [1.0, float("nan")])
@pytest.mark.parametrize("mx", CLIPS)
def test_a_flagged_step_leaves_the_step_counts_and_the_next_one_proceeds(mx, flag):
    """7: found_inf set at the second of three calls (one gradient element is inf there, as it would be): no bit of p, m, v or
    state['step'] changes, skipped_steps == 1, and the third call gives, bit for bit, what an optimizer that never saw the second
    gives -- its bias correction is that of step 2, which a count of calls kept on the host would make 3."""
    params, opt = W.make(mx)
    W.set_amp(opt, grad_scale=S16, found_inf=0.0)
    _step(params, opt, 0, scale=S16)
    after1 = W.state(params, opt)
    W.assert_same(after1, _plain(mx)[0][0])

    W.set_amp(opt, grad_scale=S16, found_inf=flag)
    W.set_lr(opt, 1)
    W.set_grads(params, _grads(S16)[1])
    params["w4097"].grad[4001] = float("inf")
    opt.step()
    W.assert_same(W.state(params, opt), after1)
    assert all(float(opt.state[params[n]]["step"]) == (0.0 if n == "empty" else 1.0) for n in W.with_grad(1))
    assert int(opt.skipped_steps) == 1
    if mx is not None:   # the norm is still written
        assert torch.isinf(opt.last_grad_norm).item()

    W.set_amp(opt, grad_scale=S16, found_inf=0.0)
    _step(params, opt, 2, scale=S16)
    want, want_norm = _plain(mx, steps=(0, 2))[1]
    W.assert_same(W.state(params, opt), want)
    assert float(opt.state[params["w4097"]]["step"]) == 2.0 and float(opt.state[params["late"]]["step"]) == 1.0
    if mx is not None:
        np.testing.assert_array_equal(_norm_bits(opt), want_norm)
    assert int(opt.skipped_steps) == 1
    # and that trajectory is not the one a count of calls gives: the bias corrections of steps 2 and 3 differ in fp32
    assert W.step_size(U.group_lr(1, 2), W.BETAS, 2, True) != W.step_size(U.group_lr(1, 2), W.BETAS, 3, True)


@pytest.mark.parametrize("mx", CLIPS)
def test_a_flagged_first_step_creates_zero_state_with_step_zero(mx):
    """8"""
    params, opt = W.make(mx)
    W.set_amp(opt, grad_scale=S16, found_inf=1.0)
    _step(params, opt, 0, scale=S16)
    got, P = W.state(params, opt), W.init_params()
    for n in W.NAMES:
        np.testing.assert_array_equal(got[n][0], P[n], err_msg=n)
        if n in W.with_grad(0):
            assert not got[n][1].any() and not got[n][2].any() and got[n][3] == 0.0, n
        else:
            assert len(got[n]) == 1
    assert int(opt.skipped_steps) == 1
    W.set_amp(opt, grad_scale=S16, found_inf=0.0)   # the next step is the plain first step
    opt.step()
    W.assert_same(W.state(params, opt), _plain(mx)[0][0])


@pytest.mark.parametrize("mx", CLIPS)
def test_a_nan_gradient_poisons_its_own_tensor_or_with_clipping_every_tensor(mx):
    """9: ordinary NaN values in one gradient.  Without clipping only that tensor turns NaN and the others keep the plain step's
    bits; with clipping the total norm and the clip factor are NaN and every stepped tensor with elements is."""
    params, opt = W.make(mx)
    W.set_lr(opt, 0)
    W.set_grads(params, _grads()[0])
    params["w4097"].grad[17] = float("nan")
    opt.step()
    got, want = W.state(params, opt), _plain(mx)[0][0]
    assert np.isnan(got["w4097"][0][17]) and np.isnan(got["w4097"][1][17]) and np.isnan(got["w4097"][2][17])
    for n in W.with_grad(0):
        if n in ("w4097", "empty"):
            continue
        if mx is None:
            for x, y in zip(got[n], want[n]):
                np.testing.assert_array_equal(x, y, err_msg=n)
        else:
            assert np.isnan(got[n][0]).all() and np.isnan(got[n][1]).all(), n
    if mx is None:
        assert not np.isnan(np.delete(got["w4097"][0], 17)).any()
    else:
        assert torch.isnan(opt.last_grad_norm).item()
    np.testing.assert_array_equal(got["no_grad"][0], W.init_params()["no_grad"])


def _scaler():
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16)
    scaler.scale(torch.zeros((), device=DEV))   # the scaler creates its scale tensor at the first scale() call
    return scaler


@pytest.mark.parametrize("mx", CLIPS)
def test_scaler_step_and_plain_step_read_nothing_back_to_the_host(mx, monkeypatch):
    """10: through a real torch.amp.GradScaler, with Tensor.item raising inside scaler.step(opt) and opt.step()."""
    scaler = _scaler()
    params, opt = W.make(mx)
    p2, o2 = W.make(mx)
    for ps, o in ((params, opt), (p2, o2)):
        W.set_lr(o, 0)
    W.set_grads(params, _grads(S16)[0])
    W.set_grads(p2, _grads()[0])

    def no_item(self):
        raise AssertionError("Tensor.item() called inside the step: a host wait")

    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "item", no_item)
        scaler.step(opt)
        o2.step()
    scaler.update()
    W.assert_same(W.state(params, opt), _plain(mx)[0][0])
    W.assert_same(W.state(p2, o2), _plain(mx)[0][0])
    assert not hasattr(opt, "grad_scale") and not hasattr(opt, "found_inf")
    # an inf gradient: the scaler's own check sets found_inf, the step is skipped on the device and update() halves the scale
    W.set_lr(opt, 1)
    W.set_grads(params, _grads(S16)[1])
    params["w768x768"].grad.view(-1)[300000] = float("inf")
    before = W.state(params, opt)
    scaler.step(opt)
    scaler.update()
    W.assert_same(W.state(params, opt), before)
    assert int(opt.skipped_steps) == 1 and scaler.get_scale() == S16 / 2


@pytest.mark.parametrize("mx", CLIPS)
def test_after_scaler_unscale_only_found_inf_is_honoured(mx):
    """11: scaler.unscale_(opt) first: grad_scale arrives as None, and the bits are the plain step's on the unscaled gradients."""
    scaler = _scaler()
    params, opt = W.make(mx)
    seen = []
    step = opt.step

    def spy(*a, **kw):
        seen.append((opt.grad_scale, opt.found_inf))
        return step(*a, **kw)

    opt.step = spy
    for t, (want, want_norm) in enumerate(_plain(mx)):
        W.set_lr(opt, t)
        W.set_grads(params, _grads(S16)[t])
        scaler.unscale_(opt)
        scaler.step(opt)
        scaler.update()
        W.assert_same(W.state(params, opt), want)
        if mx is not None:
            np.testing.assert_array_equal(_norm_bits(opt), want_norm)
    assert len(seen) == 3 and all(gs is None and fi is not None and fi.numel() == 1 for gs, fi in seen)
    assert int(opt.skipped_steps) == 0
    W.set_grads(params, _grads(S16)[0])   # an inf found by unscale_ skips the step as well
    params["one"].grad[0] = float("inf")
    before = W.state(params, opt)
    scaler.unscale_(opt)
    scaler.step(opt)
    scaler.update()
    W.assert_same(W.state(params, opt), before)
    assert int(opt.skipped_steps) == 1 and scaler.get_scale() == S16 / 2


def test_resume_from_its_own_file_and_from_the_reference_layout(golden_dir):
    """12: stop after step 2, torch.save(state_dict()): the step entries are Python ints; a fresh optimizer loads the file and
    continues bit for bit as the uninterrupted run.  Then the reference's layout (CPU tensors, int steps) built from the golden's
    state after step 2 (the 768 x 768 tensor, sampled there, from the fp64 restatement rounded to fp32), stepped to 5."""
    whole = _plain(None, steps=(0, 1, 2, 3, 4))
    params, opt = W.make()
    for t in (0, 1):
        _step(params, opt, t)
    sd = opt.state_dict()
    assert all(type(s["step"]) is int for s in sd["state"].values())
    assert {W.PACKED[i]: s["step"] for i, s in sd["state"].items()} == {n: (0 if n == "empty" else 2) for n in W.with_grad(1)}
    assert all(isinstance(opt.state[params[n]]["step"], torch.Tensor) for n in W.with_grad(1))
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    after2 = W.state(params, opt)
    p2, o2 = W.make(start={n: (after2[n][0],) for n in W.NAMES})
    o2.load_state_dict(torch.load(buf, weights_only=True))
    assert all(o2.state[p2[n]]["step"].is_cuda and o2.state[p2[n]]["exp_avg"].is_cuda for n in W.with_grad(1))
    for t in (2, 3, 4):
        _step(p2, o2, t)
        W.assert_same(W.state(p2, o2), whole[t][0])

    j, g = _golden(golden_dir)
    traj = W.run_fp64(5)
    T0 = 2
    start, state = {}, {}
    for i, name in enumerate(W.PACKED):
        if name not in traj[T0 - 1][2]:
            continue
        shape = W.init_params()[name].shape
        if U.recorded(name, np.zeros(shape)).size == int(np.prod(shape)):
            p, m, v = (g["cb.%s.%d.%s" % (name, T0 - 1, k)].reshape(shape) for k in ("p", "m", "v"))
        else:
            p, m, v = (traj[T0 - 1][2][name][k].astype(np.float32) for k in range(3))
        step = W.layout_at(j, "cb", T0 - 1)["step"][str(i)]
        assert type(step) is int and step == T0
        # the fused step never advances the count of a tensor of no elements; the restatement resumes from the same count
        start[name] = (p, m, v, 0 if p.size == 0 else step)
        state[i] = dict(step=step, exp_avg=torch.from_numpy(np.array(m)), exp_avg_sq=torch.from_numpy(np.array(v)))
    pgs = [dict(pg, betas=tuple(pg["betas"])) for pg in W.layout_at(j, "cb", T0 - 1)["param_groups"]]
    p3, o3 = W.make(start=start)
    o3.load_state_dict({"state": state, "param_groups": pgs})
    assert all(o3.state[p3[n]]["exp_avg"].is_cuda and o3.state[p3[n]]["step"].is_cuda for n in start)
    assert "late" not in start and p3["late"] not in o3.state
    got = []
    for t in range(T0, 5):
        _step(p3, o3, t)
        got.append(W.state(p3, o3))
    want = W.run_fp64(5, start=start, first=T0)
    # the loaded count of the empty tensor is the reference's 2 and stays: only compare where there are elements
    for rec in got:
        rec["empty"][3] = np.float32(0.0)
    _check_against_oracle(got, [None] * T0 + want, g, "cb", range(T0, 5), 5)


def test_wrong_scalars_and_a_non_contiguous_gradient_are_refused_by_name():
    """13"""
    params, opt = W.make(1.0, names=["w1023", "three"])
    W.set_grads(params, _grads()[0])
    keep = W.state(params, opt)
    good = torch.zeros((), dtype=torch.float32, device=DEV)
    for attr in ("found_inf", "grad_scale"):
        other = "grad_scale" if attr == "found_inf" else "found_inf"
        for bad in (torch.zeros(()), torch.zeros((), dtype=torch.int32, device=DEV), torch.zeros(2, device=DEV),
                    torch.zeros((), dtype=torch.float64, device=DEV), 0.0):
            setattr(opt, attr, bad)
            setattr(opt, other, good + (1.0 if other == "grad_scale" else 0.0))
            with pytest.raises(_lib.AnceLibraryError, match=r"AdamW: optimizer\.%s" % attr):
                opt.step()
    opt.grad_scale = opt.found_inf = None
    params["w1023"].grad = torch.zeros(2046, device=DEV)[::2]
    with pytest.raises(_lib.AnceLibraryError, match=r"AdamW: param_groups\[0\]\['params'\]\[0\]\.grad must be contiguous"):
        opt.step()
    for n in params:   # nothing was stepped
        np.testing.assert_array_equal(params[n].detach().cpu().numpy(), keep[n][0])
    assert opt.last_grad_norm is None and len(opt.state) == 0   # a refused call leaves no state behind
