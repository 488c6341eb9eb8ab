"""The replayable training step on the GPU: the device-resident dropout stream (ance_amd.attention.dropout_state.to_device /
advance, the *_dstream entry points of include/ance_amd.h) under every dropout kernel, eager and replayed from a captured graph.

Every comparison here is bit for bit: a call under the device stream {s, b} with relative index r must draw what the host-valued
call at (seed, offset) = (s, b + r) draws, and nothing else in the kernels differs."""
import ctypes

import numpy as np
import pytest
import torch

import train_step_util as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = S.SEED
STREAM_CASES = ((0, 0), (5, 3), (2 ** 32 - 1, 2))   # (base, r); the last carries into the offset's high word
HALF = {"fp16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture(autouse=True)
def _host_mode_afterwards():
    """dropout_state is one object for the process: every test here leaves it in host mode, as the rest of the suite expects."""
    from ance_amd import attention as T
    yield
    T.dropout_state.to_host(0)
    T.manual_seed(SEED)


def _rand(tag, shape, scale=1.0, dtype=torch.float32):
    from oracle.encoder_ref import det_normal
    return torch.from_numpy(det_normal(91, tag, shape, scale)).to(DEV).to(dtype)


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).contiguous().view(torch.uint8),
                                                                           b.reshape(-1).contiguous().view(torch.uint8))


def _host_call(fn, seed, offset):
    """fn() in host mode at (seed, offset)."""
    from ance_amd import attention as T
    T.dropout_state.to_host(0)
    T.manual_seed(seed)
    T.dropout_state.offsets[0] = offset
    out = [t.clone() for t in fn()]
    assert T.dropout_state.offsets[0] == offset + 1
    return out


def _device_call(fn, seed, base, r):
    """fn() in device mode under the stream {seed, base} as the call of relative index r."""
    from ance_amd import attention as T
    T.dropout_state.to_host(0)
    T.manual_seed(seed)
    T.dropout_state.offsets[0] = base
    stream = T.dropout_state.to_device(0)
    assert stream.dtype == torch.int64 and stream.data_ptr() % 16 == 0
    assert [v & (2 ** 64 - 1) for v in stream.tolist()] == [seed, base]
    T.dropout_state.offsets[0] = r
    d_stream, rel = T.dropout_state.next_pair(torch.device(DEV))   # what a call is handed: (the tensor, r)
    assert d_stream is stream and rel == r
    T.dropout_state.offsets[0] = r
    out = [t.clone() for t in fn()]
    assert T.dropout_state.to_host(0) == (seed, base + r + 1)      # the read-back counts every call so far
    return out


# ---------------------------------------------------------------------------------------------------------------- the entry points
def _attention_case(form, precision, p):
    """12 heads, lengths (33, 5, 1) in L = 40: forward and the three gradients."""
    from ance_amd.attention import attention_packed, attention_padded
    lens, L, H = (33, 5, 1), 40, 768
    dt = torch.float32 if precision == "fp32" else HALF[precision]
    if form == "padded":
        shape = (len(lens), L, H)
    else:
        shape = (sum(lens), H)
    q, k, v, d = (_rand("attn." + n, shape, 1.0, dt) for n in "qkvd")
    lens_t = torch.tensor(lens, dtype=torch.int32, device=DEV)
    off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=DEV)
    prec = "fp32" if precision == "fp32" else "half"

    def fn():
        a, b, c = (t.clone().requires_grad_(True) for t in (q, k, v))
        if form == "padded":
            out = attention_padded(a, b, c, lens_t, 12, p, True, precision=prec)
        else:
            out = attention_packed(a, b, c, off, L, 12, p, True, precision=prec)
        out.backward(d)
        return [out.detach(), a.grad, b.grad, c.grad]
    return fn


def _first_row_case(precision, p):
    """The first-row core on the padded case's shape: q0 [3, 768], k, v [3, 40, 768]; ctx0 and the three gradients."""
    from ance_amd.attention import attention_first_row
    lens, L, H = (33, 5, 1), 40, 768
    dt = torch.float32 if precision == "fp32" else HALF[precision]
    q0, d = _rand("row0.q", (len(lens), H), 1.0, dt), _rand("row0.d", (len(lens), H), 1.0, dt)
    k, v = (_rand("row0." + n, (len(lens), L, H), 1.0, dt) for n in "kv")
    lens_t = torch.tensor(lens, dtype=torch.int32, device=DEV)

    def fn():
        a, b, c = (t.clone().requires_grad_(True) for t in (q0, k, v))
        out = attention_first_row(a, b, c, lens_t, 12, p, True, precision="fp32" if precision == "fp32" else "half")
        out.backward(d)
        return [out.detach(), a.grad, b.grad, c.grad]
    return fn


def _tail_case(H, precision, p, rows=17):
    from ance_amd.layers import dropout_add_layer_norm
    dt = torch.float32 if precision == "fp32" else HALF[precision]
    x, res, dy = _rand("tail.x", (rows, H), 1.0, dt), _rand("tail.r", (rows, H)), _rand("tail.dy", (rows, H))
    bias, g, be = _rand("tail.b", (H,), 0.1), 1.0 + _rand("tail.g", (H,), 0.1), _rand("tail.be", (H,), 0.1)

    def fn():
        ts = [t.clone().requires_grad_(True) for t in (x, bias, res, g, be)]
        y = dropout_add_layer_norm(*ts, 1e-5, p, True, precision="fp32" if precision == "fp32" else "half")
        y.backward(dy)
        return [y.detach()] + [t.grad for t in ts]
    return fn


def _embed_case(p, rows=17, H=768):
    from ance_amd.embeddings import bert_embeddings
    ids = torch.from_numpy(np.random.default_rng(3).integers(1, 50, size=(1, rows))).to(DEV)
    word, pos, typ = _rand("emb.w", (50, H), 0.5), _rand("emb.p", (40, H), 0.1), _rand("emb.t", (2, H), 0.1)
    g, be, dy = 1.0 + _rand("emb.g", (H,), 0.1), _rand("emb.be", (H,), 0.1), _rand("emb.dy", (1, rows, H))

    def fn():
        ts = [t.clone().requires_grad_(True) for t in (word, pos, typ, g, be)]
        y = bert_embeddings(ids, *ts, 1e-5, padding_idx=0, dropout_p=p, training=True)
        y.backward(dy)
        return [y.detach()] + [t.grad for t in ts]
    return fn


ENTRY_POINTS = (
    [("attention %s %s" % (f, pr), lambda p, f=f, pr=pr: _attention_case(f, pr, p)) for f in ("padded", "packed") for pr in ("fp32", "fp16", "bf16")]
    + [("first row %s" % pr, lambda p, pr=pr: _first_row_case(pr, p)) for pr in ("fp32", "fp16", "bf16")]
    + [("tail %d %s" % (H, pr), lambda p, H=H, pr=pr: _tail_case(H, pr, p)) for H in (768, 1024) for pr in ("fp32", "fp16", "bf16")]
    + [("embeddings", lambda p: _embed_case(p))])


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("name,make", ENTRY_POINTS, ids=[n for n, _ in ENTRY_POINTS])
def test_device_stream_draws_the_host_calls_bits(name, make, p):
    """d_stream = {s, b} with relative index r against the host-valued call at (s, b + r): the forward output and every gradient
    bit for bit, for every dropout entry point, (b, r) in STREAM_CASES (the last carries into the high word).  The masks of
    different offsets differ, so the equality is not one of a constant."""
    fn = make(p)
    firsts = []
    for base, r in STREAM_CASES:
        want = _host_call(fn, SEED, base + r)
        got = _device_call(fn, SEED, base, r)
        assert len(want) == len(got)
        for i, (a, b) in enumerate(zip(want, got)):
            assert _bits_equal(a, b), (name, p, base, r, i)
        firsts.append(want[0])
    assert not _bits_equal(firsts[0], firsts[1]) and not _bits_equal(firsts[1], firsts[2])


def test_unaligned_stream_is_refused_and_nothing_is_launched():
    from ance_amd import _lib
    L = _lib.lib()
    buf = torch.zeros(4, dtype=torch.int64, device=DEV)
    bad = ctypes.c_void_p(buf.data_ptr() + 8)
    st = _lib.current_stream_ptr()
    calls = [("ance_attention_forward_dstream", (ctypes.byref(_lib.AnceAttnTrainArgs()),)),
             ("ance_attention_backward_dstream", (ctypes.byref(_lib.AnceAttnTrainArgs()), ctypes.byref(_lib.AnceAttnGradArgs()))),
             ("ance_attention16_forward_dstream", (ctypes.byref(_lib.AnceAttn16Args()),)),
             ("ance_attention16_backward_dstream", (ctypes.byref(_lib.AnceAttn16Args()), ctypes.byref(_lib.AnceAttn16GradArgs()))),
             ("ance_attention_row0_forward_dstream", (ctypes.byref(_lib.AnceAttn16Args()),)),
             ("ance_attention_row0_backward_dstream", (ctypes.byref(_lib.AnceAttn16Args()), ctypes.byref(_lib.AnceAttn16GradArgs()))),
             ("ance_layer_tail_forward_dstream", (ctypes.byref(_lib.AnceLayerTailArgs()),)),
             ("ance_layer_tail_backward_dstream", (ctypes.byref(_lib.AnceLayerTailArgs()), ctypes.byref(_lib.AnceLayerTailGradArgs()))),
             ("ance_layer_tail16_forward_dstream", (ctypes.byref(_lib.AnceLayerTail16Args()),)),
             ("ance_layer_tail16_backward_dstream", (ctypes.byref(_lib.AnceLayerTail16Args()), ctypes.byref(_lib.AnceLayerTail16GradArgs()))),
             ("ance_embed_forward_dstream", (ctypes.byref(_lib.AnceEmbedArgs()),)),
             ("ance_embed_backward_dstream", (ctypes.byref(_lib.AnceEmbedArgs()), ctypes.byref(_lib.AnceEmbedGradArgs())))]
    for name, structs in calls:
        assert getattr(L, name)(*structs, bad, st) == _lib.ANCE_E_INVALID, name
        msg = L.ance_last_error().decode()
        assert name in msg and "d_stream" in msg, msg
    assert L.ance_dropout_stream_advance(bad, 1, st) == _lib.ANCE_E_INVALID
    torch.cuda.synchronize()
    assert not buf.any()


# ---------------------------------------------------------------------------------------------------------------- replays
def _replay_case(fn, n_replays=3):
    """fn's forward + backward, then advance(), captured once in device mode and replayed: replay k against the eager host-mode call
    at offset k, every output bit for bit; the first outputs of the replays differ from one another."""
    from ance_amd import attention as T
    want = [_host_call(fn, SEED, k) for k in range(n_replays)]
    T.dropout_state.to_host(0)
    T.manual_seed(SEED)
    T.dropout_state.to_device(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up on a side stream; it ends with its own advance, so the capture starts at r = 0
        fn()
        T.dropout_state.advance(0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    T.dropout_state.to_host(0)
    T.manual_seed(SEED)             # back to {SEED, 0}: replay k stands for the call at offset k
    T.dropout_state.to_device(0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = fn()
        T.dropout_state.advance(0)
    assert T.dropout_state.offsets[0] == 0
    got = []
    for k in range(n_replays):
        for t in outs:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got.append([t.clone() for t in outs])
        for i, (a, b) in enumerate(zip(want[k], got[k])):
            assert _bits_equal(a, b), (k, i)
    assert T.dropout_state.to_host(0) == (SEED, n_replays)
    for a in range(n_replays):
        for b in range(a + 1, n_replays):
            assert not _bits_equal(got[a][0], got[b][0]), (a, b)


def test_replays_advance_the_masks_layer_tail():
    """dropout_add_layer_norm, p = 0.1, 17 rows: y and all five gradients of replay k are those of the eager call at offset k."""
    _replay_case(_tail_case(768, "fp32", 0.1))


def test_replays_advance_the_masks_attention():
    _replay_case(_attention_case("padded", "fp32", 0.1))


def test_replays_advance_the_masks_embeddings():
    _replay_case(_embed_case(0.1))


def test_backward_after_advance_is_refused():
    """Eager, device mode: forward, advance(), backward.  The base has moved, the backward would regenerate another mask."""
    from ance_amd import _lib
    from ance_amd import attention as T
    from ance_amd.layers import dropout_add_layer_norm
    H = 768
    T.manual_seed(SEED)
    T.dropout_state.to_device(0)
    ts = [t.requires_grad_(True) for t in (_rand("ba.x", (17, H)), _rand("ba.b", (H,)), _rand("ba.r", (17, H)), _rand("ba.g", (H,)),
                                           _rand("ba.be", (H,)))]
    y = dropout_add_layer_norm(*ts, 1e-5, 0.1, True)
    T.dropout_state.advance(0)
    with pytest.raises(_lib.AnceLibraryError, match="dropout stream has moved"):
        y.backward(torch.ones_like(y))
    # without the advance in between the same backward runs
    y = dropout_add_layer_norm(*ts, 1e-5, 0.1, True)
    y.backward(torch.ones_like(y))
    T.dropout_state.advance(0)
    T.dropout_state.advance(0)   # r is 0: nothing is enqueued
    assert T.dropout_state.to_host(0) == (SEED, 2)


# ---------------------------------------------------------------------------------------------------------------- eager: both modes
def _dev_calls(calls):
    return [(torch.from_numpy(c["ids"]).to(DEV), None if c["types"] is None else torch.from_numpy(c["types"]).to(DEV),
             torch.from_numpy(c["lens"]).to(DEV)) for c in calls]


def _triplet_step(tower, dcalls):
    from ance_amd.loss import nll_loss
    loss = nll_loss(*[tower(*c) for c in dcalls])
    loss.backward()
    return loss


def test_eager_step_is_the_same_in_both_modes():
    """The BASE tower (N = 2, H 768), one triplet step at p = 0.1, in host mode and in device mode without any advance: the loss
    and every gradient bit for bit."""
    from ance_amd import attention as T
    cfg = S.BASE
    tower = S.device_tower(cfg, S.tower_state(cfg), 0.1).train()
    dcalls = _dev_calls(S.step_calls(cfg, "triplet", 0))
    res = {}
    for mode in ("host", "device"):
        T.dropout_state.to_host(0)
        T.manual_seed(SEED)
        if mode == "device":
            T.dropout_state.to_device(0)
        tower.zero_grad(set_to_none=True)
        loss = _triplet_step(tower, dcalls)
        res[mode] = [loss.detach().clone()] + [q.grad.clone() for q in tower.parameters()]
        assert T.dropout_state.offsets[0] == 3 * S.draws_per_call(cfg)
    assert len(res["host"]) == len(res["device"]) == 1 + len(S.param_names(cfg))
    for i, (a, b) in enumerate(zip(res["host"], res["device"])):
        assert _bits_equal(a, b), i


# ---------------------------------------------------------------------------------------------------------------- the resident plan
PLAN_SHAPES = ((1,), (1023,), (4097,), (768, 768))
PLAN_KERNELS = {("Lamb", False): 3, ("Lamb", True): 5, ("AdamW", False): 2, ("AdamW", True): 3}


def _traced(fn):
    """(kernel launches, copies) of one call, counted as scripts/bench_adamw.py's traced_launches does."""
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


def _plan_optimizer(kind, clip, lr=None):
    """Two groups over PLAN_SHAPES (group 0: the first two tensors, no decay; group 1: the rest), seeded parameters."""
    from ance_amd import optim
    ps = [torch.nn.Parameter(_rand("plan.p%d" % i, s, 0.5)) for i, s in enumerate(PLAN_SHAPES)]
    lrs = lr or (1e-3, 2e-3)
    groups = [dict(params=ps[:2], lr=lrs[0], weight_decay=0.0), dict(params=ps[2:], lr=lrs[1], weight_decay=0.01)]
    opt = getattr(optim, kind)(groups, betas=(0.9, 0.999), eps=1e-6, max_grad_norm=1.0 if clip else None)
    return ps, opt


def _set_grads(ps, step, fresh=()):
    """Seeded gradients of a step, written in place (the pointers stay); `fresh`: indices that get a new tensor instead."""
    keep = []
    for i, p in enumerate(ps):
        if not p.requires_grad:
            p.grad = None
            continue
        g = _rand("plan.g%d.%d" % (i, step), p.shape, 0.1)
        if p.grad is None or i in fresh:
            keep.append(p.grad)   # the old tensor stays allocated while the new one is made: another pointer
            p.grad = None         # set to None and back
            p.grad = g.clone()
        else:
            p.grad.copy_(g)
    return keep


def _opt_state(ps, opt):
    out = []
    for p in ps:
        st = opt.state.get(p) or {}
        out.append([p.detach().clone()] + [st[k].detach().clone() for k in ("exp_avg", "exp_avg_sq") if k in st]
                   + ([st["step"].detach().clone()] if isinstance(st.get("step"), torch.Tensor) else []))
    return out


def _same_state(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y), i
        for j, (s, t) in enumerate(zip(x, y)):
            assert _bits_equal(s, t), (i, j)


@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
@pytest.mark.parametrize("kind", ["Lamb", "AdamW"])
def test_resident_plan(kind, clip):
    """Five steps against a twin that calls invalidate_plan() before every step: parameters, moments and AdamW's step counts bit
    for bit; from the second step on the plan object is the same, the traced step copies nothing and launches exactly 3 / 5 / 2 / 3
    kernels; then every change the key must see rebuilds the plan and the step after it equals the twin's."""
    from ance_amd import _lib
    ps, opt = _plan_optimizer(kind, clip)
    qs, twin = _plan_optimizer(kind, clip)
    sends = _lib.lib().ance_debug_staging_sends()
    plans = []
    for t in range(5):
        _set_grads(ps, t)
        _set_grads(qs, t)
        twin.invalidate_plan()
        twin.step()
        if t in (1, 4):
            kernels, copies = _traced(opt.step)
            assert copies == 0 and len(kernels) == PLAN_KERNELS[(kind, clip)], (t, copies, kernels)
        else:
            opt.step()
        plans.append(opt._plan)
        _same_state(_opt_state(ps, opt), _opt_state(qs, twin))
    assert all(p is plans[0] for p in plans) and twin._plan is not plans[0]
    assert _lib.lib().ance_debug_staging_sends() == sends   # no step here went through the shared staging pool

    def rebuilt_step(t, **kw):
        old = opt._plan
        _set_grads(ps, t, **kw)
        _set_grads(qs, t, **kw)
        twin.invalidate_plan()
        twin.step()
        opt.step()
        assert opt._plan is not old and opt._plan.key != old.key, t
        _same_state(_opt_state(ps, opt), _opt_state(qs, twin))
        again = opt._plan
        _set_grads(ps, t + 100)
        _set_grads(qs, t + 100)
        twin.invalidate_plan()
        twin.step()
        opt.step()
        assert opt._plan is again
        _same_state(_opt_state(ps, opt), _opt_state(qs, twin))

    rebuilt_step(5, fresh=(2,))   # a gradient set to None and back: a new pointer
    for xs in (ps, qs):   # a parameter frozen
        xs[1].requires_grad_(False)
    rebuilt_step(6)
    for o in (opt, twin):
        o.param_groups[1]["weight_decay"] = 0.02
    rebuilt_step(7)
    for o in (opt, twin):
        o.param_groups[0]["lr"] = 3e-3
    rebuilt_step(8)


@pytest.mark.parametrize("kind", ["Lamb", "AdamW"])
def test_device_lr(kind):
    """A 0-dim float64 device-tensor lr steps to the bits of the float lr; lr.fill_(x) between steps takes effect with the plan
    object unchanged and equals a float-x step."""
    dlr = tuple(torch.tensor(v, dtype=torch.float64, device=DEV) for v in (1e-3, 2e-3))
    ps, opt = _plan_optimizer(kind, True, dlr)
    qs, ref = _plan_optimizer(kind, True)
    for t in range(2):
        _set_grads(ps, t)
        _set_grads(qs, t)
        opt.step()
        ref.step()
        _same_state(_opt_state(ps, opt), _opt_state(qs, ref))
    plan = opt._plan
    for x0, x1 in ((7e-4, 1.3e-3), (0.1, 1e-7)):
        dlr[0].fill_(x0)
        dlr[1].fill_(x1)
        ref.param_groups[0]["lr"], ref.param_groups[1]["lr"] = x0, x1
        _set_grads(ps, 9)
        _set_grads(qs, 9)
        opt.step()
        ref.step()
        assert opt._plan is plan
        _same_state(_opt_state(ps, opt), _opt_state(qs, ref))
    from ance_amd import _lib
    opt.param_groups[0]["lr"] = torch.tensor(1e-3, device=DEV)   # fp32: refused, not read back
    with pytest.raises(_lib.AnceLibraryError, match="float64"):
        opt.step()


# ---------------------------------------------------------------------------------------------------------------- the schedule
def _lambda_lr(base_lrs, warm, total):
    from transformers import get_linear_schedule_with_warmup
    sgd = torch.optim.SGD([dict(params=[torch.nn.Parameter(torch.zeros(1))], lr=b) for b in base_lrs], lr=1.0)
    return sgd, get_linear_schedule_with_warmup(sgd, warm, total)


@pytest.mark.parametrize("warm,total,steps", [(2, 5, 8), (0, 3, 5)])
def test_schedule_on_the_device(warm, total, steps):
    """Each group's lr tensor after each step() equals LambdaLR over transformers' lambda with == on float64; one launch per
    step(); state_dict round trip."""
    from ance_amd.optim import LinearWarmupSchedule
    base = (1e-6, 5e-6)
    ps, opt = _plan_optimizer("Lamb", False, base)
    sched = LinearWarmupSchedule(opt, warm, total)
    sgd, want = _lambda_lr(base, warm, total)
    lrs = [g["lr"] for g in opt.param_groups]
    assert all(isinstance(lr, torch.Tensor) and lr.dtype == torch.float64 and lr.dim() == 0 and lr.is_cuda for lr in lrs)
    assert sched.base_lrs == list(base)
    assert [lr.item() for lr in lrs] == want.get_last_lr() == sched.get_last_lr()    # n = 0 at construction
    for n in range(1, steps + 1):
        sgd.step()
        want.step()
        if n == 2:
            kernels, copies = _traced(sched.step)
            assert len(kernels) == 1 and copies == 0, (kernels, copies)
        else:
            sched.step()
        got = [g["lr"].item() for g in opt.param_groups]
        assert got == want.get_last_lr(), (n, got, want.get_last_lr())
        assert all(g["lr"] is lr for g, lr in zip(opt.param_groups, lrs))   # changed in place: the optimizer's plan stays
    sd = sched.state_dict()
    assert sd["last_epoch"] == steps == want.state_dict()["last_epoch"] and sd["_last_lr"] == want.get_last_lr()
    _, opt2 = _plan_optimizer("Lamb", False, base)
    other = LinearWarmupSchedule(opt2, 1, 2)
    other.load_state_dict(sd)
    assert other.get_last_lr() == sched.get_last_lr() and other.state_dict() == sd
    other.step()
    sched.step()
    assert other.get_last_lr() == sched.get_last_lr()


# ---------------------------------------------------------------------------------------------------------------- whole steps
_STATES = {}


def _tower_state(cfg):
    key = cfg["H"]
    if key not in _STATES:
        _STATES[key] = S.tower_state(cfg)
    return _STATES[key]


def _calls_of(cfg, kind, t):
    if kind == "triplet":
        return S.batches(cfg, t, S.TRIPLET_SEEDS[t % len(S.TRIPLET_SEEDS)])
    return S.inbatch_calls(S.batches(cfg, t, S.INBATCH_SEEDS[t % len(S.INBATCH_SEEDS)]), cfg["pad"])


def _loss(kind, embs):
    from ance_amd.loss import biencoder_nll_loss, nll_loss
    if kind == "triplet":
        return nll_loss(*embs)
    return biencoder_nll_loss(embs[0], embs[1], torch.arange(len(embs[0]), device=DEV))[0]


def _setup(cfg, kind, precision="fp32"):
    from ance_amd import optim
    import lamb_util as U
    tower = S.device_tower(cfg, _tower_state(cfg), 0.1, precision=precision).train()
    Opt = optim.Lamb if kind == "triplet" else optim.AdamW
    opt = Opt(S.param_groups(tower), lr=1e-3, betas=U.BETAS, eps=U.EPS, max_grad_norm=1.0)
    return tower, opt


def _snapshot(tower, opt):
    out = []
    for q in tower.parameters():
        st = opt.state[q]
        out.append((q.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()))
    return out


def _fwd_bwd(tower, dcalls, kind, autocast):
    with torch.autocast("cuda", dtype=autocast or torch.bfloat16, enabled=autocast is not None):
        loss = _loss(kind, [tower(*c) for c in dcalls])
    loss.backward()
    return loss


def _eager_run(cfg, kind, steps, device_mode, precision="fp32", autocast=None, sync_check_at=None):
    """`steps` whole steps run eagerly.  Host mode: a float lr driven by transformers' get_linear_schedule_with_warmup (the parent's
    way); device mode: LinearWarmupSchedule, the resident plan and advance().  Returns the snapshots after every step and the
    embeddings' output of the first call of every step."""
    from transformers import get_linear_schedule_with_warmup
    from ance_amd import attention as T
    from ance_amd.optim import LinearWarmupSchedule
    tower, opt = _setup(cfg, kind, precision)
    T.dropout_state.to_host(0)
    T.manual_seed(SEED)
    if device_mode:
        T.dropout_state.to_device(0)
        sched = LinearWarmupSchedule(opt, 2, 5)
    else:
        sched = get_linear_schedule_with_warmup(opt, 2, 5)
    snaps = []
    for t in range(steps):
        dcalls = _dev_calls(_calls_of(cfg, kind, t))
        torch.cuda.synchronize()
        prev = torch.cuda.get_sync_debug_mode()
        if t == sync_check_at:
            torch.cuda.set_sync_debug_mode("error")   # any synchronising torch call raises
        try:
            _fwd_bwd(tower, dcalls, kind, autocast)
            opt.step()
            sched.step()
            T.dropout_state.advance(0)
        finally:
            torch.cuda.set_sync_debug_mode(prev)
        snaps.append(_snapshot(tower, opt))
        opt.zero_grad(set_to_none=True)
    return snaps


def test_no_synchronisation_in_a_device_mode_step():
    """One whole eager step in device mode with plan and schedule under set_sync_debug_mode("error") -- the third, so that the
    optimizer's state exists."""
    _eager_run(S.BASE, "triplet", 3, True, sync_check_at=2)


def _graph_run(cfg, kind, steps, precision="fp32", autocast=None):
    """The capture recipe of INTEGRATION.md: to_device; warm-up steps on a side stream; zero_grad(set_to_none=True); capture forward,
    objective, backward, optimizer.step(), schedule.step(), advance(); static inputs fed by copy_; replay.  The warm-up steps are
    real steps, so everything they moved is put back in place before the capture (the test compares from step 0)."""
    from ance_amd import _lib
    from ance_amd import attention as T
    from ance_amd.optim import LinearWarmupSchedule
    tower, opt = _setup(cfg, kind, precision)
    T.dropout_state.to_host(0)
    T.manual_seed(SEED)
    T.dropout_state.to_device(0)
    sched = LinearWarmupSchedule(opt, 2, 5)
    static = _dev_calls(_calls_of(cfg, kind, 0))
    start = [q.detach().clone() for q in tower.parameters()]
    sends = _lib.lib().ance_debug_staging_sends()

    def step():
        _fwd_bwd(tower, static, kind, autocast)
        opt.step()
        sched.step()
        T.dropout_state.advance(0)

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
            if isinstance(st["step"], torch.Tensor):
                st["step"].zero_()
    sched.load_state_dict(dict(last_epoch=0))
    T.manual_seed(SEED)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    snaps = []
    for t in range(steps):
        for dst, src in zip(static, _dev_calls(_calls_of(cfg, kind, t))):
            for a, b in zip(dst, src):
                if a is not None:
                    a.copy_(b)
        graph.replay()
        torch.cuda.synchronize()
        snaps.append(_snapshot(tower, opt))
    assert _lib.lib().ance_debug_staging_sends() == sends, "a table upload went through the shared staging pool"
    assert T.dropout_state.to_host(0) == (SEED, steps * len(static) * S.draws_per_call(cfg))
    assert sched.state_dict()["last_epoch"] == steps
    return snaps


def _assert_same_runs(want, got, names):
    assert len(want) == len(got)
    for t, (a, b) in enumerate(zip(want, got)):
        for n, x, y in zip(names, a, b):
            for k, (s, u) in enumerate(zip(x, y)):
                assert _bits_equal(s, u), "step %d %s %s: max |d| %.3e" % (t, n, "pmv"[k], float((s.double() - u.double()).abs().max()))


@pytest.mark.parametrize("which", ["base_triplet_lamb", "large_inbatch_adamw"])
def test_whole_step_captured_and_replayed(which):
    """Step 0 captured by the recipe, replayed for steps 0 - 3 with the inputs copied in: after every replay every parameter and
    both moments equal, bit for bit, the same four steps run eagerly in HOST mode with transformers'
    get_linear_schedule_with_warmup driving a float lr -- the dropout masks, the learning rates and the clipped update of the step
    each replay stands for.  No table upload goes through the shared staging pool."""
    cfg, kind = (S.BASE, "triplet") if which == "base_triplet_lamb" else (S.LARGE, "inbatch")
    want = _eager_run(cfg, kind, 4, False)
    got = _graph_run(cfg, kind, 4)
    _assert_same_runs(want, got, S.param_names(cfg))
    for t in range(1, 4):   # the steps differ from one another: the equality is not one of a stuck state
        assert not _bits_equal(got[t][0][0], got[t - 1][0][0])


def test_whole_step_captured_bf16_autocast():
    """The BASE case under torch.autocast(bf16) with precision="half" and no scaler: the replays against the same steps run eagerly
    in device mode, bit for bit."""
    cfg, kind = S.BASE, "triplet"
    want = _eager_run(cfg, kind, 4, True, precision="half", autocast=torch.bfloat16)
    got = _graph_run(cfg, kind, 4, precision="half", autocast=torch.bfloat16)
    _assert_same_runs(want, got, S.param_names(cfg))
