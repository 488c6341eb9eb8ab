"""The fused LAMB step under loss scaling on the GPU (ance_amd.optim.Lamb under torch.amp.GradScaler -> ance_lamb_step_amp,
csrc/lamb.hip): a power-of-two scale against the plain step bit for bit (which tests/golden/lamb*.npz and objective.npz pin to the
reference's own Lamb), a general scale against "torch unscales, then the plain step", the skip on the device, and the whole thing
through a real GradScaler without a host read.  Fixture: tests/lamb_util.py's SPEC (sizes 0, 1, 3, 1023, 4097 and a 36-chunk tensor,
two groups, a None gradient)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import amp_util as A
import lamb_util as U
from ance_amd import _lib

pytestmark = pytest.mark.gpu

DEV = A.DEV
S16 = 65536.0
CLIPS = [1.0, None]   # the fixture's gradient norm is ~7.7: 1.0 clips at every step


@functools.lru_cache(maxsize=None)
def _plain(max_grad_norm, steps=(0, 1, 2)):
    """The existing step (ance_lamb_step / ance_lamb_step_clipped) on the fixture's own gradients, at the given steps' gradients and
    learning rates: per step (state, last_grad_norm bits or None).  Computed once, never changed."""
    params, opt = A.make(max_grad_norm)
    out = []
    for t in steps:
        A.set_lr(opt, t)
        A.set_grads(params, t)
        opt.step()
        out.append((A.state(params, opt), None if opt.last_grad_norm is None else opt.last_grad_norm.cpu().numpy().copy()))
    assert opt.skipped_steps is None
    return out


def _norm_bits(opt):
    return None if opt.last_grad_norm is None else opt.last_grad_norm.cpu().numpy()


@pytest.mark.parametrize("mx", CLIPS)
def test_power_of_two_scale_is_bit_neutral(mx):
    params, opt = A.make(mx)
    A.set_amp(opt, grad_scale=S16, found_inf=0.0)
    for t, (want, want_norm) in enumerate(_plain(mx)):
        A.set_lr(opt, t)
        A.set_grads(params, t, scale=S16)
        before = {n: params[n].grad.clone() for n in A.WITH_GRAD}
        opt.step()
        A.assert_same(A.state(params, opt), want)
        for n in A.WITH_GRAD:   # p.grad keeps its (scaled) bits
            assert torch.equal(params[n].grad, before[n]), n
            assert torch.equal(params[n].grad, torch.from_numpy(U.grad(n, t)).to(DEV) * S16), n
        if mx is None:
            assert opt.last_grad_norm is None
        else:
            np.testing.assert_array_equal(_norm_bits(opt), want_norm)
    assert int(opt.skipped_steps) == 0 and opt.skipped_steps.dtype == torch.int64 and opt.skipped_steps.dim() == 0


@pytest.mark.parametrize("mx", CLIPS)
def test_general_scale_equals_torch_unscaling_then_the_existing_step(mx):
    """grad_scale = 1000: array_equal to multiplying every gradient by inv = float32(1 / float64(1000)) with torch (an fp32 product,
    element by element) and then the existing plain / clipped step.  last_grad_norm within 1 ulp of the fp64 norm of those products:
    one rounding of an fp64 sum, as in tests/test_gpu_lamb_clip.py."""
    scale = 1000.0
    inv = torch.tensor(float(A.inv_scale(scale)), dtype=torch.float32, device=DEV)
    assert inv.cpu().numpy() == A.inv_scale(scale) and float(inv) * scale != 1.0   # not a power of two: the product rounds
    pa, oa = A.make(mx)
    pr, orf = A.make(mx)
    A.set_amp(oa, grad_scale=scale, found_inf=0.0)
    for t in range(3):
        for params, opt in ((pa, oa), (pr, orf)):
            A.set_lr(opt, t)
            A.set_grads(params, t, scale=scale)
        before = {n: pa[n].grad.clone() for n in A.WITH_GRAD}
        for n in A.WITH_GRAD:
            pr[n].grad = pr[n].grad * inv
            np.testing.assert_array_equal(pr[n].grad.cpu().numpy(), A.unscaled(A.scaled_grad(n, t, scale), scale), err_msg=n)
        oa.step()
        orf.step()
        A.assert_same(A.state(pa, oa), A.state(pr, orf))
        for n in A.WITH_GRAD:
            assert torch.equal(pa[n].grad, before[n]), n
        if mx is not None:
            want = A.grad_norm_fp64(t, scale)
            print("step %d: norm %.9g (fp64 %.12g)" % (t, float(oa.last_grad_norm), want))
            assert torch.equal(oa.last_grad_norm, orf.last_grad_norm)
            assert abs(float(oa.last_grad_norm) - want) <= U.ulp32(want)
            assert 7.0 < want < 8.0


@pytest.mark.parametrize("flag", [1.0, float("nan")])
@pytest.mark.parametrize("mx", CLIPS)
def test_a_flagged_step_changes_nothing_and_the_next_one_proceeds(mx, flag):
    """found_inf set at step 2 of 3 (one gradient element is inf there, as it would be): p, m, v keep their bits, the recorded norms
    stay step 1's, skipped_steps == 1, and step 3 gives what an optimizer that never saw step 2 gives."""
    params, opt = A.make(mx)
    A.set_amp(opt, grad_scale=S16, found_inf=0.0)
    A.set_lr(opt, 0)
    A.set_grads(params, 0, scale=S16)
    opt.step()
    after1 = A.state(params, opt)
    A.assert_same(after1, _plain(mx)[0][0])

    A.set_amp(opt, grad_scale=S16, found_inf=flag)
    A.set_lr(opt, 1)
    A.set_grads(params, 1, scale=S16)
    params["w4097"].grad[4001] = float("inf")
    opt.step()
    A.assert_same(A.state(params, opt), after1)
    assert int(opt.skipped_steps) == 1
    if mx is not None:   # the norm is still written
        assert torch.isinf(opt.last_grad_norm).item()

    A.set_amp(opt, grad_scale=S16, found_inf=0.0)
    A.set_lr(opt, 2)
    A.set_grads(params, 2, scale=S16)
    opt.step()
    want, want_norm = _plain(mx, steps=(0, 2))[1]
    A.assert_same(A.state(params, opt), want)
    if mx is not None:
        np.testing.assert_array_equal(_norm_bits(opt), want_norm)
    assert int(opt.skipped_steps) == 1
    assert all(opt.state[params[n]]["step"] == 3 for n in A.WITH_GRAD)   # calls, the skipped one included


@pytest.mark.parametrize("mx", CLIPS)
def test_a_flagged_first_step_creates_zero_state_and_leaves_the_parameters(mx):
    params, opt = A.make(mx)
    A.set_amp(opt, grad_scale=S16, found_inf=1.0)
    A.set_lr(opt, 0)
    A.set_grads(params, 0, scale=S16)
    opt.step()
    got, P = A.state(params, opt), U.init_params()
    for n in A.NAMES:
        np.testing.assert_array_equal(got[n][0], P[n], err_msg=n)
        if n in A.WITH_GRAD:
            assert not got[n][1].any() and not got[n][2].any(), n
            np.testing.assert_array_equal(got[n][3], np.array([0, 0, 1], np.float32), err_msg=n)
        else:
            assert len(got[n]) == 1
    assert int(opt.skipped_steps) == 1
    # the next step is the plain first step
    A.set_amp(opt, grad_scale=S16, found_inf=0.0)
    opt.step()
    A.assert_same(A.state(params, opt), _plain(mx)[0][0])


def _scaler():
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16)
    scaler.scale(torch.zeros((), device=DEV))   # the scaler creates its scale tensor at the first scale() call
    return scaler


def _scaler_run(mx):
    """Through a real GradScaler with hand-set gradients: steps 0 and 1 finite, then step 2's gradients with one inf element (skipped,
    the scale halves), then step 2's gradients at the halved scale.  Returns what each call left."""
    scaler = _scaler()
    params, opt = A.make(mx)
    seen = []
    for t, bad in ((0, False), (1, False), (2, True), (2, False)):
        scale = scaler.get_scale()
        A.set_lr(opt, t)
        A.set_grads(params, t, scale=scale)
        if bad:
            params["w768x768"].grad.view(-1)[300000] = float("inf")
        assert not hasattr(opt, "grad_scale") and not hasattr(opt, "found_inf")
        scaler.step(opt)
        scaler.update()
        seen.append((scale, A.state(params, opt), _norm_bits(opt), int(opt.skipped_steps)))
    return seen


@pytest.mark.parametrize("mx", CLIPS)
def test_through_a_real_grad_scaler(mx):
    seen = _scaler_run(mx)
    plain = _plain(mx)
    assert [s[0] for s in seen] == [S16, S16, S16, S16 / 2]        # (b) update() halves the scale after the inf
    assert [s[3] for s in seen] == [0, 0, 1, 1]
    for k in (0, 1):                                                # (a) finite steps: the plain run's bits
        A.assert_same(seen[k][1], plain[k][0])
        if mx is not None:
            np.testing.assert_array_equal(seen[k][2], plain[k][1])
    A.assert_same(seen[2][1], seen[1][1])                           # (b) the inf step changed nothing
    A.assert_same(seen[3][1], plain[2][0])                          # ... and the next finite step proceeds
    if mx is not None:
        np.testing.assert_array_equal(seen[3][2], plain[2][1])


@pytest.mark.parametrize("mx", CLIPS)
def test_after_scaler_unscale_only_found_inf_is_honoured(mx):
    """(c) scaler.unscale_(opt) first: grad_scale arrives as None, and the bits are the plain step's on the unscaled gradients."""
    scaler = _scaler()
    params, opt = A.make(mx)
    seen_scale = []
    step = opt.step

    def spy(*a, **kw):
        seen_scale.append((opt.grad_scale, opt.found_inf))
        return step(*a, **kw)

    opt.step = spy
    for t, (want, want_norm) in enumerate(_plain(mx)):
        A.set_lr(opt, t)
        A.set_grads(params, t, scale=S16)
        scaler.unscale_(opt)
        for n in A.WITH_GRAD:
            assert torch.equal(params[n].grad, torch.from_numpy(U.grad(n, t)).to(DEV)), n
        scaler.step(opt)
        scaler.update()
        A.assert_same(A.state(params, opt), want)
        if mx is not None:
            np.testing.assert_array_equal(_norm_bits(opt), want_norm)
    assert len(seen_scale) == 3 and all(gs is None and fi is not None and fi.numel() == 1 for gs, fi in seen_scale)
    assert int(opt.skipped_steps) == 0
    # an inf found by unscale_ skips the step as well
    A.set_grads(params, 0, scale=S16)
    params["one"].grad[0] = float("inf")
    before = A.state(params, opt)
    scaler.unscale_(opt)
    scaler.step(opt)
    scaler.update()
    A.assert_same(A.state(params, opt), before)
    assert int(opt.skipped_steps) == 1 and scaler.get_scale() == S16 / 2


def test_the_fused_clip_sees_the_unscaled_gradients_without_unscale():
    """The trap this removes: Lamb(max_grad_norm=1.0) under the scaler without scaler.unscale_ must clip by, and report, the norm of
    the unscaled gradients (~7.7, not ~5e5).  Within 1 ulp of the fp64 norm: one rounding of an fp64 sum."""
    scaler = _scaler()
    params, opt = A.make(1.0)
    A.set_lr(opt, 0)
    A.set_grads(params, 0, scale=S16)
    scaler.step(opt)
    scaler.update()
    want = A.grad_norm_fp64(0, S16)
    print("norm %.9g (fp64 of the unscaled gradients %.12g)" % (float(opt.last_grad_norm), want))
    assert 7.0 < want < 8.0
    assert abs(float(opt.last_grad_norm) - want) <= U.ulp32(want)


@pytest.mark.parametrize("mx", CLIPS)
def test_scaler_step_reads_nothing_back_to_the_host(mx, monkeypatch):
    scaler = _scaler()
    params, opt = A.make(mx)
    A.set_lr(opt, 0)
    A.set_grads(params, 0, scale=S16)

    def no_item(self):
        raise AssertionError("Tensor.item() called inside scaler.step(optimizer): a host wait")

    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "item", no_item)
        scaler.step(opt)
    scaler.update()
    A.assert_same(A.state(params, opt), _plain(mx)[0][0])


def test_deterministic():
    a, b = _scaler_run(1.0), _scaler_run(1.0)
    for x, y in zip(a, b):
        assert x[0] == y[0] and x[3] == y[3]
        A.assert_same(x[1], y[1])
        np.testing.assert_array_equal(x[2], y[2])


def test_a_wrong_found_inf_or_grad_scale_is_refused_by_name():
    params, opt = A.make(1.0, names=["w1023", "three"])
    A.set_grads(params, 0)
    keep = A.state(params, opt)
    good = torch.zeros((), dtype=torch.float32, device=DEV)
    for attr in ("found_inf", "grad_scale"):
        other = "grad_scale" if attr == "found_inf" else "found_inf"
        for bad in (torch.zeros(()), torch.zeros((), dtype=torch.int32, device=DEV), torch.zeros(2, device=DEV),
                    torch.zeros((), dtype=torch.float64, device=DEV), 0.0):
            setattr(opt, attr, bad)
            setattr(opt, other, good + (1.0 if other == "grad_scale" else 0.0))
            with pytest.raises(_lib.AnceLibraryError, match=r"optimizer\.%s" % attr):
                opt.step()
    for n in params:   # nothing was stepped
        np.testing.assert_array_equal(params[n].detach().cpu().numpy(), keep[n][0])
    assert opt.last_grad_norm is None


@pytest.mark.parametrize("mx", CLIPS)
def test_without_the_two_pointers_the_new_entry_gives_the_existing_entries_bits(mx):
    """ance_lamb_step_amp called directly with d_grad_scale = d_found_inf = d_prev_out = d_skipped = NULL."""
    L = _lib.lib()
    names = A.WITH_GRAD
    P = U.init_params()
    p = [torch.from_numpy(np.ascontiguousarray(P[n], np.float32)).to(DEV) for n in names]
    g = [torch.from_numpy(U.grad(n, 0)).to(DEV) for n in names]
    m, v = [torch.zeros_like(x) for x in p], [torch.zeros_like(x) for x in p]
    gi = {n: k for n, _, k, _, _ in U.SPEC}
    T = (_lib.AnceLambTensor * len(names))()
    for i, n in enumerate(names):
        T[i].p, T[i].g, T[i].m, T[i].v = p[i].data_ptr(), g[i].data_ptr(), m[i].data_ptr(), v[i].data_ptr()
        T[i].numel, T[i].group = p[i].numel(), gi[n]
    G = (_lib.AnceLambGroup * 2)()
    for k in range(2):
        G[k].lr, G[k].beta1, G[k].beta2, G[k].eps = U.group_lr(k, 0), U.BETAS[0], U.BETAS[1], U.EPS
        G[k].weight_decay = U.GROUPS[k]["weight_decay"]
    need = L.ance_lamb_amp_workspace_bytes(len(names), 2, sum(x.numel() for x in p))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.empty((len(names), 3), dtype=torch.float32, device=DEV)
    norm = torch.full((1,), -1.0, dtype=torch.float32, device=DEV)
    rc = L.ance_lamb_step_amp(T, len(names), G, 2, 0, 0.0 if mx is None else mx, None, None, None,
                              None if mx is None else ctypes.c_void_p(norm.data_ptr()), None, ctypes.c_void_p(out.data_ptr()),
                              ctypes.c_void_p(ws.data_ptr()), need, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "ance_lamb_step_amp")
    want, want_norm = _plain(mx)[0]
    for i, n in enumerate(names):
        for got, w in zip((p[i], m[i], v[i], out[i]), want[n]):
            np.testing.assert_array_equal(got.cpu().numpy(), w, err_msg=n)
    if mx is not None:
        np.testing.assert_array_equal(norm[0].cpu().numpy(), want_norm)
