"""The device-resident loss scaler on the GPU (ance_amd.optim.LossScaler; ance_lamb_step_scaled, ance_adamw_step_scaled and
ance_loss_scale_update of include/ance_amd.h): the step that finds its own overflow against the same optimizer driven the way
torch.amp.GradScaler drives it, a trajectory whose scales are known in advance, the scale's update against torch's op, the launch,
copy and synchronisation counts, and the fp16 tower eager and replayed from one captured graph.

Every comparison is bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import loss_scaler_util as U
import train_step_util as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = S.SEED
CHUNK = 16384
# the parameters of the synthetic cases: around one chunk, three chunks, and one tensor that begins one element into its storage
# (4 bytes past a 16-byte boundary: the non-vector path).  Group 0: the first three (no decay); group 1: the rest.
SIZES = (3, 1, 1001, 16383, 16384, 16385, 32773)
ONE, UNALIGNED, BIG, LAST = 1, 2, 6, 6
INF, NAN = float("inf"), float("nan")
# name -> (tensor, element, value, the steps of three it is planted in)
GRAD_CASES = {
    "clean": None,
    "inf first element of the first tensor": (0, 0, INF, (0, 1)),
    "nan last element of the last tensor": (LAST, SIZES[LAST] - 1, NAN, (1,)),
    "-inf last element of chunk 0": (BIG, CHUNK - 1, -INF, (1,)),
    "-inf first element of chunk 1": (BIG, CHUNK, -INF, (1,)),
    "inf in the one-element tensor": (ONE, 0, INF, (1,)),
    "nan last element of the unaligned tensor": (UNALIGNED, SIZES[UNALIGNED] - 1, NAN, (1,)),
}
KERNELS = {"Lamb": 5, "AdamW": 3}


@pytest.fixture(autouse=True)
def _host_mode_afterwards():
    """dropout_state is one object for the process: every test here leaves it in host mode, as the rest of the suite expects."""
    from ance_amd import attention as T
    yield
    T.dropout_state.to_host(0)
    T.manual_seed(SEED)


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).contiguous().view(torch.uint8),
                                                                           b.reshape(-1).contiguous().view(torch.uint8))


def _randn(seed, n, scale):
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)).to(DEV)


_START = {}


def _start_values():
    """The parameters' start values, made once and never changed."""
    if not _START:
        _START["p"] = [_randn(100 + i, n, 0.5) for i, n in enumerate(SIZES)]
    return _START["p"]


def _optimizer(kind, clip):
    from ance_amd import optim
    ps = []
    for i, (n, v) in enumerate(zip(SIZES, _start_values())):
        if i == UNALIGNED:
            store = torch.zeros(n + 1, dtype=torch.float32, device=DEV)
            store[1:].copy_(v)
            p = torch.nn.Parameter(store[1:])
            assert p.data_ptr() % 16 == 4 and p.is_contiguous()
        else:
            p = torch.nn.Parameter(v.clone())
        ps.append(p)
    groups = [dict(params=ps[:3], lr=1e-3, weight_decay=0.0), dict(params=ps[3:], lr=2e-3, weight_decay=0.01)]
    return ps, getattr(optim, kind)(groups, betas=(0.9, 0.999), eps=1e-6, max_grad_norm=1.0 if clip else None)


def _set_grads(ps, step, scale, case):
    """Seeded gradients of a step times the loss scale, written in place; the case's element planted in its steps."""
    for i, p in enumerate(ps):
        g = _randn(1000 + 10 * step + i, p.numel(), 0.05) * scale
        if p.grad is None:
            p.grad = g.clone()
        else:
            p.grad.copy_(g)
    if case is not None and step in case[3]:
        ps[case[0]].grad[case[1]] = case[2]


def _state(ps, opt):
    out = []
    for p in ps:
        st = opt.state[p]
        out.append([p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
                   + [st[k].detach().clone().reshape(1) for k in ("step", "weight_norm", "adam_norm", "trust_ratio")
                      if isinstance(st.get(k), torch.Tensor)])
    norm = opt.last_grad_norm
    out.append([torch.zeros(0, device=DEV) if norm is None else norm.detach().clone().reshape(1), opt.skipped_steps.clone().reshape(1)])
    return out


def _assert_same(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y), (what, i)
        for j, (s, t) in enumerate(zip(x, y)):
            assert _bits_equal(s, t), (what, i, j)


def _scaler(scale, **kw):
    from ance_amd.optim import LossScaler
    scaler = LossScaler(init_scale=scale, **kw)
    scaler.scale(torch.zeros((), device=DEV))   # creates the device state
    return scaler


# ------------------------------------------------------------------------------------------------ against the parent's path
@pytest.mark.parametrize("clip", [True, False], ids=["clip", "plain"])
@pytest.mark.parametrize("kind", ["Lamb", "AdamW"])
def test_scaled_step_equals_the_step_driven_as_gradscaler_drives_it(kind, clip):
    """Three consecutive steps per gradient case and scale.  The parent's path: the same class with optimizer.grad_scale set and
    optimizer.found_inf set to what torch computes from isfinite over the gradients.  LossScaler.step must leave every p, m, v,
    AdamW's step, LAMB's recorded rows, last_grad_norm (NaN included) and skipped_steps with the same bits, and its flag must be
    that flag."""
    for scale in (65536.0, 3.0):
        for name, case in GRAD_CASES.items():
            ps, opt = _optimizer(kind, clip)
            qs, ref = _optimizer(kind, clip)
            scaler = _scaler(scale)
            ref_scale = torch.full((1,), scale, dtype=torch.float32, device=DEV)
            flags = []
            for t in range(3):
                _set_grads(ps, t, scale, case)
                _set_grads(qs, t, scale, case)
                bad = any(not bool(torch.isfinite(q.grad).all()) for q in qs)
                ref.grad_scale, ref.found_inf = ref_scale, torch.full((1,), float(bad), dtype=torch.float32, device=DEV)
                ref.step()
                ref.grad_scale = ref.found_inf = None
                scaler.step(opt)
                flags.append(bad)
                assert scaler.found_inf.item() == float(bad), (scale, name, t)
                _assert_same(_state(ps, opt), _state(qs, ref), (scale, name, t))
            assert flags == [case is not None and t in case[3] for t in range(3)], (scale, name)
            assert opt.skipped_steps.item() == sum(flags)
            assert not _bits_equal(ps[BIG].detach(), _start_values()[BIG])   # the applied steps moved the parameters


@pytest.mark.parametrize("clip", [True, False], ids=["clip", "plain"])
@pytest.mark.parametrize("kind", ["Lamb", "AdamW"])
def test_scale_below_one_flags_a_finite_gradient_whose_product_overflows(kind, clip):
    """Scale 0.5, every gradient finite, one element 3e38: g * inv = 6e38 is inf in fp32.  torch's check of g sees nothing; the
    step's own flag is 1, the step is skipped and no bit changes."""
    ps, opt = _optimizer(kind, clip)
    scaler = _scaler(0.5)
    _set_grads(ps, 0, 0.5, None)
    scaler.step(opt)
    assert scaler.found_inf.item() == 0.0 and opt.skipped_steps.item() == 0
    before = _state(ps, opt)
    _set_grads(ps, 1, 0.5, (4, 77, 3e38, (1,)))
    assert all(bool(torch.isfinite(p.grad).all()) for p in ps)
    scaler.step(opt)
    assert scaler.found_inf.item() == 1.0 and opt.skipped_steps.item() == 1
    after = _state(ps, opt)
    if clip:
        assert torch.isinf(after[-1][0]).all()
        before[-1][0] = after[-1][0]   # last_grad_norm is the one thing a skipped step writes
    before[-1][1] = after[-1][1]
    _assert_same(before, after, "skipped")


# ------------------------------------------------------------------------------------------------ a trajectory known in advance
OVERFLOW_STEPS = (1, 2, 6)


def _trajectory(kind, driver, steps=10, sync_check_at=None, traced_at=None):
    """loss = (sum_i (w_i * x_i).sum()) * mult, mult 3e38 at OVERFLOW_STEPS (every gradient is then non-finite) and 1 otherwise.
    Returns (the scale after each step, the final tracker, skipped_steps, the final state, [(kernels, copies)] of traced_at)."""
    from ance_amd.optim import LossScaler
    ps, opt = _optimizer(kind, True)
    xs = [_randn(500 + i, n, 1.0) for i, n in enumerate(SIZES)]
    mult = torch.ones((), dtype=torch.float32, device=DEV)
    if driver == "ours":
        scaler = LossScaler(init_scale=65536.0, growth_interval=2)
    else:
        scaler = torch.amp.GradScaler("cuda", init_scale=65536.0, growth_interval=2)
    scales, traced = [], []
    for t in range(steps):
        mult.fill_(3e38 if t in OVERFLOW_STEPS else 1.0)
        torch.cuda.synchronize()
        prev = torch.cuda.get_sync_debug_mode()
        if t == sync_check_at:
            torch.cuda.set_sync_debug_mode("error")
        try:
            loss = sum((w * x).sum() for w, x in zip(ps, xs)) * mult
            scaler.scale(loss).backward()
            if t == traced_at:
                traced.append(_traced(lambda: scaler.step(opt)))
                traced.append(_traced(scaler.update))
            else:
                scaler.step(opt)
                scaler.update()
        finally:
            torch.cuda.set_sync_debug_mode(prev)
        if t in OVERFLOW_STEPS:
            assert all(not bool(torch.isfinite(p.grad).any()) for p in ps)
        scales.append(scaler.get_scale())
        opt.zero_grad(set_to_none=False)   # in place: the plan stays resident
    if driver == "ours":
        tracker, s_bits = scaler.growth_tracker.clone(), scaler.scale_tensor.clone()
    else:
        tracker, s_bits = scaler._growth_tracker.clone().reshape(1), scaler._scale.clone().reshape(1)
    return scales, tracker, s_bits, opt.skipped_steps.item(), _state(ps, opt), traced


@pytest.mark.parametrize("kind", ["Lamb", "AdamW"])
def test_trajectory_follows_the_rule_and_gradscaler(kind):
    """Ten steps, init_scale 65536, growth_interval 2, overflows at steps 1, 2 and 6: the scale after each step is the schedule
    the rule gives, the tracker ends at 1 and three steps are skipped; a torch.amp.GradScaler run of the same steps with the same
    optimizer class ends in the same bits everywhere, the scaler's state included."""
    scales, tracker, s_bits, skipped, state, _ = _trajectory(kind, "ours")
    assert scales == [2.0 ** e for e in (16, 15, 14, 14, 15, 15, 14, 14, 15, 15)] == U.schedule(65536.0, OVERFLOW_STEPS, 10)[0]
    assert tracker.item() == 1 and skipped == 3
    t_scales, t_tracker, t_bits, t_skipped, t_state, _ = _trajectory(kind, "torch")
    assert t_scales == scales and t_skipped == skipped
    assert _bits_equal(tracker, t_tracker) and _bits_equal(s_bits, t_bits)
    _assert_same(state, t_state, "final state")


# ------------------------------------------------------------------------------------------------ the scale's update
def test_scale_update_is_torchs_op_on_the_device():
    """ance_loss_scale_update against torch._amp_update_scale_ on device tensors over the CPU table, and both against the rule."""
    from ance_amd import _lib
    L, table = _lib.lib(), U.cases()
    n = len(table)
    ours_s = torch.tensor([c[0] for c in table], dtype=torch.float32, device=DEV)
    ours_t = torch.tensor([c[1] for c in table], dtype=torch.int32, device=DEV)
    flags = torch.tensor([c[2] for c in table], dtype=torch.float32, device=DEV)
    want_s, want_t = ours_s.clone(), ours_t.clone()
    st = _lib.current_stream_ptr()
    for i, (_, _, _, gf, bf, interval) in enumerate(table):
        _lib.check(L.ance_loss_scale_update(ctypes.c_void_p(ours_s.data_ptr() + 4 * i), ctypes.c_void_p(ours_t.data_ptr() + 4 * i),
                                            ctypes.c_void_p(flags.data_ptr() + 4 * i), gf, bf, interval, st), "ance_loss_scale_update")
        torch._amp_update_scale_(want_s[i:i + 1], want_t[i:i + 1], flags[i:i + 1], gf, bf, interval)
    torch.cuda.synchronize()
    assert _bits_equal(ours_s, want_s) and _bits_equal(ours_t, want_t)
    rule = [U.update_rule(*c) for c in table]
    assert [U.bits32(s) for s, _ in rule] == [U.bits32(s) for s in ours_s.tolist()] and [t for _, t in rule] == ours_t.tolist()
    assert n == 72 and not _bits_equal(ours_s, torch.tensor([c[0] for c in table], dtype=torch.float32, device=DEV))


# ------------------------------------------------------------------------------------------------ launches, copies, host waits
def _traced(fn):
    """(kernel launches, copies) of one call, counted as tests/test_gpu_graph_step.py's _traced does."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    kernels, copies = [], 0
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            if "memcpy" in e.name.lower() or "memset" in e.name.lower():
                copies += 1
            elif not e.name.startswith("Optimizer.step"):
                kernels.append(e.name)
    return kernels, copies


@pytest.mark.parametrize("clip", [True, False], ids=["clip", "plain"])
@pytest.mark.parametrize("kind", ["Lamb", "AdamW"])
def test_launch_and_copy_counts(kind, clip):
    """With a resident plan a scaled step enqueues at most 5 (LAMB) / 3 (AdamW) kernels and no copy, with and without the clip;
    update() enqueues one kernel and no copy."""
    ps, opt = _optimizer(kind, clip)
    scaler = _scaler(65536.0)
    for t in range(3):
        _set_grads(ps, t, 65536.0, None)
        if t < 2:
            scaler.step(opt)
            scaler.update()
            continue
        plan = opt._plan
        kernels, copies = _traced(lambda: scaler.step(opt))
        assert opt._plan is plan and copies == 0 and 1 <= len(kernels) <= KERNELS[kind], (kernels, copies)
        kernels, copies = _traced(scaler.update)
        assert copies == 0 and len(kernels) == 1, (kernels, copies)
    # a step with and a step without the scaler do not share a plan
    _set_grads(ps, 3, 1.0, None)
    opt.step()
    assert opt._plan is not plan and opt._plan.key != plan.key


@pytest.mark.parametrize("kind", ["Lamb", "AdamW"])
def test_no_synchronisation_in_scale_backward_step_update(kind):
    """scale -> backward -> step -> update of the third step under set_sync_debug_mode("error")."""
    _trajectory(kind, "ours", steps=3, sync_check_at=2)


def test_update_with_a_new_scale_and_checkpoint_round_trip():
    """update(new_scale) fills the device scalar in place (a host tensor is refused during capture); state_dict() loads into
    torch.amp.GradScaler and back; loading fills the device tensors in place."""
    from ance_amd import _lib
    scaler = _scaler(65536.0, growth_interval=3)
    ptrs = (scaler.scale_tensor.data_ptr(), scaler.growth_tracker.data_ptr(), scaler.found_inf.data_ptr())
    scaler.update(1024.0)
    assert scaler.get_scale() == 1024.0
    scaler.update(torch.tensor(3.0, device=DEV))
    assert scaler.get_scale() == 3.0
    scaler.update(torch.tensor([7.0]))   # from the host: allowed outside a capture
    assert scaler.get_scale() == 7.0
    scaler.update()
    sd = scaler.state_dict()
    assert sd == dict(scale=7.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3, _growth_tracker=1)
    theirs = torch.amp.GradScaler("cuda")
    theirs.load_state_dict(sd)
    assert theirs.state_dict() == sd
    theirs.scale(torch.zeros((), device=DEV))
    assert theirs.state_dict() == sd
    back = _scaler(2.0)
    back.load_state_dict(theirs.state_dict())
    assert back.state_dict() == sd and back.scale_tensor.item() == 7.0 and back.growth_tracker.item() == 1
    assert ptrs == (scaler.scale_tensor.data_ptr(), scaler.growth_tracker.data_ptr(), scaler.found_inf.data_ptr())
    x = torch.full((3,), 2.0, device=DEV)
    a, b = scaler.scale([x, x[0]])
    assert a.tolist() == [14.0] * 3 and b.item() == 14.0 and b.dim() == 0
    graph = torch.cuda.CUDAGraph()
    host = torch.tensor(5.0)
    with pytest.raises(_lib.AnceLibraryError, match="cannot be captured"):
        with torch.cuda.graph(graph):
            scaler.update(2.0)   # a float is a kernel argument: captured (the graph is never replayed)
            scaler.update(host)
    assert scaler.get_scale() == 7.0


# ------------------------------------------------------------------------------------------------ the fp16 tower
TOWER_STEPS = 5
TOWER_OVERFLOWS = (1, 3)
_TOWER = {}


def _dev_calls(calls):
    return [(torch.from_numpy(c["ids"]).to(DEV), None if c["types"] is None else torch.from_numpy(c["types"]).to(DEV),
             torch.from_numpy(c["lens"]).to(DEV)) for c in calls]


def _calls_of(cfg, t):
    return S.batches(cfg, t, S.TRIPLET_SEEDS[t % len(S.TRIPLET_SEEDS)])


def _tower_setup():
    from ance_amd import optim
    import lamb_util
    cfg = S.BASE
    if "sd" not in _TOWER:
        _TOWER["sd"] = S.tower_state(cfg)
    tower = S.device_tower(cfg, _TOWER["sd"], 0.1, precision="half").train()
    opt = optim.Lamb(S.param_groups(tower), lr=1e-3, betas=lamb_util.BETAS, eps=lamb_util.EPS, max_grad_norm=1.0)
    return cfg, tower, opt


def _make_scaler(driver):
    from ance_amd.optim import LossScaler
    if driver == "ours":
        return LossScaler(init_scale=65536.0, growth_interval=2)
    return torch.amp.GradScaler("cuda", init_scale=65536.0, growth_interval=2)


def _scaler_state(scaler):
    if isinstance(scaler, torch.amp.GradScaler):
        return scaler._scale.clone().reshape(1), scaler._growth_tracker.clone().reshape(1)
    return scaler.scale_tensor.clone(), scaler.growth_tracker.clone()


def _tower_snapshot(tower, opt, scaler):
    out = []
    for q in tower.parameters():
        st = opt.state[q]
        out.append((q.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()))
    out.append(_scaler_state(scaler))
    return out


def _tower_step(tower, opt, scaler, sched, dcalls, mult):
    from ance_amd import attention as T
    from ance_amd.loss import nll_loss
    with torch.autocast("cuda", dtype=torch.float16):
        loss = nll_loss(*[tower(*c) for c in dcalls])
    scaler.scale(loss * mult).backward()
    scaler.step(opt)
    scaler.update()
    sched.step()
    T.dropout_state.advance(0)


def _tower_eager(driver):
    """Five eager steps in device mode; the snapshots after every step and skipped_steps."""
    from ance_amd import attention as T
    from ance_amd.optim import LinearWarmupSchedule
    cfg, tower, opt = _tower_setup()
    T.dropout_state.to_host(0)
    T.manual_seed(SEED)
    T.dropout_state.to_device(0)
    sched = LinearWarmupSchedule(opt, 2, 5)
    scaler = _make_scaler(driver)
    mult = torch.ones((), dtype=torch.float32, device=DEV)
    snaps = []
    for t in range(TOWER_STEPS):
        mult.fill_(3e38 if t in TOWER_OVERFLOWS else 1.0)
        _tower_step(tower, opt, scaler, sched, _dev_calls(_calls_of(cfg, t)), mult)
        snaps.append(_tower_snapshot(tower, opt, scaler))
        opt.zero_grad(set_to_none=True)
    return snaps, opt.skipped_steps.item()


def _eager_ours():
    """Run (a) with the LossScaler, computed once and shared by the two tower tests; never changed."""
    if "ours" not in _TOWER:
        _TOWER["ours"] = _tower_eager("ours")
    return _TOWER["ours"]


def _assert_same_runs(want, got):
    assert len(want) == len(got)
    for t, (a, b) in enumerate(zip(want, got)):
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            for k, (s, u) in enumerate(zip(x, y)):
                assert _bits_equal(s, u), "step %d entry %d.%d" % (t, i, k)


def test_tower_eager_equals_gradscaler():
    """(a) The fp16 BASE tower, triplet, Lamb with the clip, dropout 0.1, five steps with the loss times 3e38 on steps 1 and 3:
    every parameter, both moments, the scale and the tracker after every step equal the same steps under torch.amp.GradScaler."""
    ours, skipped = _eager_ours()
    theirs, t_skipped = _tower_eager("torch")
    _assert_same_runs(theirs, ours)
    scales = [snap[-1][0].item() for snap in ours]
    print("tower: skipped_steps %d (GradScaler %d), scale after each step %s" % (skipped, t_skipped, scales))
    assert skipped == t_skipped and skipped >= 2
    # a step that did not back the scale off was applied, and an applied step moves the parameters
    applied = [t for t in range(1, TOWER_STEPS) if scales[t] >= scales[t - 1]]
    assert len(applied) == TOWER_STEPS - 1 - sum(1 for t in range(1, TOWER_STEPS) if scales[t] < scales[t - 1])
    assert applied, "every step overflowed: nothing was applied"
    for t in applied:
        assert any(not _bits_equal(a[0], b[0]) for a, b in zip(ours[t][:-1], ours[t - 1][:-1])), t


def test_tower_step_captured_with_its_scaler():
    """(b) The capture recipe with scaler.scale(loss).backward(), scaler.step(opt), scaler.update(), sched.step() and advance() in
    one graph: warm-up steps undone in place (the scaler's three tensors included), five replays with the inputs and the multiplier
    copied in, every replay against run (a)."""
    from ance_amd import _lib
    from ance_amd import attention as T
    from ance_amd.optim import LinearWarmupSchedule
    want, want_skipped = _eager_ours()
    cfg, tower, opt = _tower_setup()
    T.dropout_state.to_host(0)
    T.manual_seed(SEED)
    T.dropout_state.to_device(0)
    sched = LinearWarmupSchedule(opt, 2, 5)
    scaler = _make_scaler("ours")
    mult = torch.ones((), dtype=torch.float32, device=DEV)
    static = _dev_calls(_calls_of(cfg, 0))
    start = [q.detach().clone() for q in tower.parameters()]
    sends = _lib.lib().ance_debug_staging_sends()

    def step():
        _tower_step(tower, opt, scaler, sched, static, mult)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
            opt.zero_grad(set_to_none=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.no_grad():   # back to step 0, in place: no pointer the plan or the graph holds changes
        for q, q0 in zip(tower.parameters(), start):
            q.copy_(q0)
            st = opt.state[q]
            st["exp_avg"].zero_()
            st["exp_avg_sq"].zero_()
        opt.skipped_steps.zero_()
    sched.load_state_dict(dict(last_epoch=0))
    scaler.load_state_dict(dict(scaler.state_dict(), scale=65536.0, _growth_tracker=0))
    scaler.found_inf.zero_()
    T.manual_seed(SEED)
    ptrs = (scaler.scale_tensor.data_ptr(), scaler.growth_tracker.data_ptr(), scaler.found_inf.data_ptr())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    assert ptrs == (scaler.scale_tensor.data_ptr(), scaler.growth_tracker.data_ptr(), scaler.found_inf.data_ptr())
    got = []
    for t in range(TOWER_STEPS):
        for dst, src in zip(static, _dev_calls(_calls_of(cfg, t))):
            for a, b in zip(dst, src):
                if a is not None:
                    a.copy_(b)
        mult.fill_(3e38 if t in TOWER_OVERFLOWS else 1.0)
        graph.replay()
        torch.cuda.synchronize()
        got.append(_tower_snapshot(tower, opt, scaler))
    _assert_same_runs(want, got)
    assert opt.skipped_steps.item() == want_skipped >= 2
    assert _lib.lib().ance_debug_staging_sends() == sends, "a table upload went through the shared staging pool"
    assert sched.state_dict()["last_epoch"] == TOWER_STEPS
