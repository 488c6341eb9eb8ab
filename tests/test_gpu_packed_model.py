"""The models of ance_amd/model.py over packed token rows (set_packed_rows) on the GPU.

  steps            BASE (N = 2, absolute positions, BiEncoder: no head, two towers) and LARGE (N = 1, RoBERTa positions, head 1024 ->
                   768: the last layer alone) at train_step_util.SHAPES, triplet and in-batch, against model_util.reference_step in
                   fp64: dropout 0 and dropout 0.1 under the REMAPPED masks (packed_util.packed_masks) -- every embedding, the loss
                   and every parameter gradient within max(4 x ref_err, 16 ulp32) (train_step_util.compare), ref_err the eager fp32
                   restatement's own distance; key.bias exactly 0.  Capacities: "exact", total + 5 and B * L
  empty sequence   a call with a length-0 sequence in the middle: finite, no gradient, the others within the same bound
  autocast         precision="half" under fp16 / bf16 autocast against the fp32 packed model: max(4 x D, 16 ulp32), D the eager
                   autocast tower's own distance (tests/test_gpu_model.py's rule)
  overflow         a capacity one row short: the dropped sequence's embedding is NaN, the others stay within the bound,
                   packed_dropped == 1, and a GradScaler + Lamb step changes no parameter bit
  capture          one captured step with int capacities replayed on three batches of different lengths and totals equals the eager
                   steps bit for bit
"""
import functools

import numpy as np
import pytest
import torch

import attention_train_util as A
import lamb_util as U
import model_util as M
import packed_util as P
import train_step_util as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = S.SEED
ROBERTA_BASE = dict(S.BASE, mode="roberta", n_types=1, pad=1)
# The seeds of train_step_util.batches at which, with these models' parameters (model_util.model_state), every triplet's negative
# leads / every query's positive trails by more than 8 in the restatement at dropout 0 and under every remapped mask set used below:
# every sequence of every call carries a full gradient (searched on the CPU; _case asserts it).  One exception: in the LARGE in-batch
# step at dropout 0 query 1, whose planted first token 777 is also its positive's, wins at every seed tried (0 .. 399); seed 31 is
# the first at which the two other queries trail by more than 8 there and all three do under the dropout masks.
BATCH_SEEDS = {("base_biencoder", "triplet"): 18, ("base_biencoder", "inbatch"): 12,
               ("large_roberta_dot", "triplet"): 41, ("large_roberta_dot", "inbatch"): 31}


@pytest.fixture(autouse=True)
def _host_mode_afterwards():
    from ance_amd import attention as T
    yield
    T.dropout_state.to_host(0)
    T.manual_seed(SEED)


def _np(t):
    return t.detach().float().cpu().numpy()


def _ids(x):
    return torch.from_numpy(np.ascontiguousarray(x)).long().to(DEV)


def _mask(lens, L):
    return (torch.arange(L)[None, :] < torch.as_tensor(np.asarray(lens))[:, None]).long().to(DEV)


def _config(cfg, p):
    from ance_amd.model import TowerConfig
    return TowerConfig(S.VOCAB, cfg["H"], cfg["N"], cfg["inter"], S.MAX_POS, cfg["n_types"], cfg["eps"], cfg["pad"], p, p, cfg["heads"])


def _load(model, sd):
    return model.to(DEV).load_reference_state_dict({k: torch.from_numpy(np.ascontiguousarray(v, np.float32)) for k, v in sd.items()})


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).contiguous().view(torch.uint8),
                                                                           b.reshape(-1).contiguous().view(torch.uint8))


def _call_args(calls):
    out = []
    for c in calls:
        out += [_ids(c["ids"]), _mask(c["lens"], c["ids"].shape[1])]
    return out


def _setup(which):
    if which == "large_roberta_dot":
        return S.LARGE, ("roberta.",) * 3, True, M.model_state(S.LARGE)
    sd = {}
    for pre, seed in (("question_model.", 73), ("ctx_model.", 74)):
        sd.update({k: v for k, v in M.model_state(S.BASE, seed, prefix=pre).items() if k.startswith(pre)})
    return S.BASE, ("question_model.", "ctx_model.", "ctx_model."), False, sd


def _model(which, p, precision="fp32"):
    from ance_amd import model
    cfg, _, head, sd = _setup(which)
    m = model.RobertaDot_NLL_LN(_config(cfg, p), precision=precision) if head else model.BiEncoder(_config(cfg, p), precision=precision)
    return _load(m, sd).train()


def _capacities(calls, rows):
    """(what set_packed_rows takes, the capacity of every call): "exact" -- every call its own total; "slack" / "full" -- total + 5
    / B * L of the query call, and ONE body capacity, that of the largest body call."""
    tot = [int(np.clip(c["lens"], 0, c["ids"].shape[1]).sum()) for c in calls]
    if rows == "exact":
        return ("exact", "exact"), tot
    src = [t + 5 for t in tot] if rows == "slack" else [c["ids"].shape[0] * c["ids"].shape[1] for c in calls]
    body = max(src[1:])
    return (src[0], body), [src[0]] + [body] * (len(calls) - 1)


def _leads(kind, embs):
    """Per triplet / query: by how much the negative leads / the positive trails the best context."""
    if kind == "triplet":
        q, a, b = (np.asarray(e, np.float64) for e in embs)
        return (q * b).sum(-1) - (q * a).sum(-1)
    q, c = (np.asarray(e, np.float64) for e in embs)
    s = q @ c.T
    return s.max(1) - s[np.arange(len(q)), np.arange(len(q))]


@functools.lru_cache(maxsize=None)
def _case(which, kind, p, rows):
    """(calls, capacities, want fp64, ref_err) of one step; the masks depend on the capacities only with dropout."""
    cfg, prefixes, head, sd = _setup(which)
    three = [dict(c, types=None) for c in S.batches(cfg, 0, BATCH_SEEDS[which, kind])]   # the models pass no token types: type 0
    calls = three if kind == "triplet" else S.inbatch_calls(three, cfg["pad"])
    prefixes = prefixes[:len(calls)]
    setting, caps = _capacities(calls, rows)
    masks = P.calls_packed_masks(p, SEED, 0, cfg, calls, caps) if p > 0 else None
    want = M.reference_step(sd, prefixes, calls, cfg, kind, masks, p, "float64", head)
    leads = _leads(kind, want["embs"])
    saturated = 1 if (which, kind, p) == ("large_roberta_dot", "inbatch", 0.0) else 0   # BATCH_SEEDS
    assert int((leads > (0 if kind == "triplet" else 8)).sum()) >= len(leads) - saturated, leads
    ref32 = M.reference_step(sd, prefixes, calls, cfg, kind, masks, p, "float32", head)
    ref_err = S.distances(ref32["grads"], want["grads"])
    ref_err["loss"] = abs(ref32["loss"] - want["loss"])
    for i in range(len(calls)):
        ref_err["emb%d" % i] = float(np.abs(ref32["embs"][i].astype(np.float64) - want["embs"][i]).max())
    return calls, setting, want, ref_err


def _step(m, kind, args):
    """(loss, embeddings) of one step through the model's public interface."""
    from ance_amd.loss import biencoder_nll_loss, nll_loss
    embs = [m.query_emb(args[0], args[1])] + [m.body_emb(args[2 * k], args[2 * k + 1]) for k in range(1, len(args) // 2)]
    if kind == "triplet":
        return nll_loss(*embs), embs
    return biencoder_nll_loss(embs[0], embs[1], torch.arange(len(embs[0]), device=DEV))[0], embs


def _check_step(tag, m, kind, calls, want, ref_err, cfg, p):
    from ance_amd import attention as T
    T.manual_seed(SEED)
    args = _call_args(calls)
    loss, embs = _step(m, kind, args)
    if p > 0:
        assert T.dropout_state.offsets[0] == len(calls) * S.draws_per_call(cfg)   # draw count and order unchanged: 1 + 3 N per call
    loss.backward()
    got = {n: _np(q.grad) for n, q in m.named_parameters()}
    assert sorted(got) == sorted(want["grads"])
    w = dict(want["grads"])
    got["loss"], w["loss"] = float(loss.detach()), want["loss"]
    for i, e in enumerate(embs):
        got["emb%d" % i], w["emb%d" % i] = _np(e), want["embs"][i]
    bad, worst = S.compare(tag, got, w, ref_err)
    print("%s largest d / bound %.3f" % (tag, worst))
    assert not bad, bad
    for n, q in m.named_parameters():
        if n.endswith("attention.self.key.bias"):
            assert not q.grad.any(), n
    return got


@pytest.mark.parametrize("which", ["base_biencoder", "large_roberta_dot"])
@pytest.mark.parametrize("kind", ["triplet", "inbatch"])
def test_packed_step_without_dropout_at_every_capacity(which, kind):
    """Dropout 0: one fp64 reference for the three capacities.  Slack rows change nothing beyond the bound: every embedding and every
    gradient of the runs with total + 5 and B * L rows is held to the same reference under the same bound."""
    cfg = _setup(which)[0]
    calls, _, want, ref_err = _case(which, kind, 0.0, "exact")
    for rows in ("exact", "slack", "full"):
        setting, _ = _capacities(calls, rows)
        m = _model(which, 0.0).set_packed_rows(*setting)
        _check_step("packed %s %s p=0 R=%s" % (which, kind, rows), m, kind, calls, want, ref_err, cfg, 0.0)
        assert int(m.packed_dropped) == 0


@pytest.mark.parametrize("which,kind,rows", [("base_biencoder", "triplet", "exact"), ("base_biencoder", "triplet", "slack"),
                                             ("base_biencoder", "triplet", "full"), ("base_biencoder", "inbatch", "slack"),
                                             ("large_roberta_dot", "triplet", "exact"), ("large_roberta_dot", "triplet", "slack"),
                                             ("large_roberta_dot", "triplet", "full"), ("large_roberta_dot", "inbatch", "slack")])
def test_packed_step_with_dropout_under_the_remapped_masks(which, kind, rows):
    """Dropout 0.1: the embeddings' and the tails' masks are those of an R-row call at the packed row index (remapped into the padded
    shape for the reference), the attention masks are the padded call's bits, the last layer's tails draw a B-row call's."""
    cfg = _setup(which)[0]
    calls, setting, want, ref_err = _case(which, kind, 0.1, rows)
    m = _model(which, 0.1).set_packed_rows(*setting)
    _check_step("packed %s %s p=0.1 R=%s" % (which, kind, rows), m, kind, calls, want, ref_err, cfg, 0.1)
    assert int(m.packed_dropped) == 0


def test_never_calling_set_packed_rows_is_the_padded_path():
    """The default and set_packed_rows() / (None, None) run the padded tower: the same bits, and no counter moves."""
    cfg = _setup("base_biencoder")[0]
    calls = [dict(c, types=None) for c in S.batches(cfg, 0, 4)]
    args = _call_args(calls)
    outs = []
    for packed in (False, True):
        from ance_amd import attention as T
        m = _model("base_biencoder", 0.1)
        if packed:
            m.set_packed_rows(5, 7).set_packed_rows()
        T.manual_seed(SEED)
        loss = m(*args)[0]
        loss.backward()
        outs.append([loss.detach()] + [p.grad for p in m.parameters()])
        assert "packed_dropped" not in m.state_dict() and not any("packed" in k for k in m.state_dict())
    assert all(_bits_equal(a, b) for a, b in zip(*outs))


# ---------------------------------------------------------------------------------------------------------------- an empty sequence
@pytest.mark.parametrize("which", ["base_biencoder", "large_roberta_dot"])
def test_an_empty_sequence_in_the_middle(which):
    """One tower call with lengths (12, 0, 5): the empty sequence's embedding is finite and NOT the padded path's value, so it is
    kept out of the objective -- the loss is sum_k <emb_k, G_k> over the two others, G fixed.  Their embeddings and every parameter
    gradient against the fp64 restatement under the usual bound; the run with five slack rows under the same one."""
    from oracle.encoder_ref import det_normal
    cfg, prefixes, head, sd = _setup(which)
    call = dict(S.batches(cfg, 0, 3)[0], types=None)
    call["lens"] = np.array([12, 0, 5], np.int32)
    call["ids"] = call["ids"].copy()
    call["ids"][np.arange(12)[None, :] >= call["lens"][:, None]] = cfg["pad"]
    some = np.array([0, 2])
    G = det_normal(5, "empty.G", (3, 768 if head else cfg["H"]), 1.0).astype(np.float64)
    ref = {}
    for dt in ("float64", "float32"):
        W = {k: torch.from_numpy(np.array(v)).to(getattr(torch, dt)).requires_grad_(True) for k, v in sd.items()}
        e = M.tower_forward(W, call, cfg, None, 0.0, prefixes[0], head)
        (e[some] * torch.from_numpy(G[some]).to(e.dtype)).sum().backward()
        ref[dt] = dict(emb=e.detach().numpy()[some], **{k: w.grad.numpy() for k, w in W.items() if w.grad is not None})
    want = ref["float64"]
    ref_err = S.distances(ref["float32"], want)
    for R in ("exact", 22):
        m = _model(which, 0.0).set_packed_rows(R, R)
        e = m.query_emb(*_call_args([call]))
        assert bool(torch.isfinite(e).all())
        (e[some] * torch.from_numpy(G[some]).float().to(DEV)).sum().backward()
        got = {n: _np(p.grad) for n, p in m.named_parameters() if p.grad is not None}
        assert sorted(got) == sorted(k for k in want if k != "emb")
        got["emb"] = _np(e)[some]
        bad, worst = S.compare("empty sequence %s R=%s" % (which, R), got, want, ref_err)
        print("empty sequence %s R=%s largest d / bound %.3f" % (which, R, worst))
        assert not bad, bad
        assert int(m.packed_dropped) == 0


# ---------------------------------------------------------------------------------------------------------------- autocast
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_half_precision_packed_model_under_autocast(dt):
    """RobertaDot_NLL_LN(precision="half"), N = 2, packed with five slack rows, under torch.autocast against the fp32 packed model,
    dropout off: tests/test_gpu_model.py's rule -- max(4 x D, 16 ulp32), D = |eager autocast tower - fp32 model| per tensor."""
    import embeddings_util as E
    import layer_half_util as HL
    import layer_tail_util as LT
    from ance_amd import model
    from ance_amd.loss import nll_loss
    dtype = torch.float16 if dt == "fp16" else torch.bfloat16
    cfg = ROBERTA_BASE
    sd = M.model_state(cfg)
    calls = S.batches(cfg, 0, 0)   # tests/test_gpu_model.py: BATCH_SEEDS["roberta_base_no_dropout"]
    args = _call_args(calls)
    setting, _ = _capacities(calls, "slack")

    def run(precision, autocast):
        m = _load(model.RobertaDot_NLL_LN(_config(cfg, 0.0), precision=precision), sd).train().set_packed_rows(*setting)
        with torch.autocast("cuda", dtype=dtype, enabled=autocast):
            embs = [m.query_emb(args[0], args[1]), m.body_emb(args[2], args[3]), m.body_emb(args[4], args[5])]
            loss = nll_loss(*embs)
        loss.backward()
        out = {n: _np(p.grad) for n, p in m.named_parameters()}
        assert all(p.grad.dtype == torch.float32 for p in m.parameters()) and all(e.dtype == torch.float32 for e in embs)
        assert int(m.packed_dropped) == 0
        out["loss"] = np.float64(float(loss.detach()))
        out.update({"emb%d" % i: _np(e) for i, e in enumerate(embs)})
        return out

    base = run("fp32", False)
    got = run("half", True)
    W = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV).requires_grad_(True) for k, v in sd.items()}
    F = torch.nn.functional
    with torch.autocast("cuda", dtype=dtype):
        embs = []
        for c in calls:
            h = E.embed_torch_forward(c["ids"], None, *(W["roberta." + n] for n in S.EMB), cfg["eps"], cfg["mode"], cfg["pad"])
            rows = torch.from_numpy(A._valid(c["lens"], c["ids"].shape[1])).to(DEV)
            for i in range(cfg["N"]):
                pre = "roberta." + S.layer_prefix(i)
                h = HL.eager_layer(h, rows, {n: W[pre + n] for n in LT.LAYER_PARAMS}, cfg["heads"], cfg["eps"])
            e = F.linear(h[:, 0], W["embeddingHead.weight"], W["embeddingHead.bias"])
            embs.append(F.layer_norm(e.float(), (768,), W["norm.weight"], W["norm.bias"], S.HEAD_EPS))
        loss = S.loss_torch("triplet", [e.float() for e in embs])
    loss.backward()
    eager = {k: _np(w.grad) for k, w in W.items()}
    eager["loss"] = np.float64(float(loss.detach()))
    eager.update({"emb%d" % i: _np(e) for i, e in enumerate(embs)})

    def logits(r):
        q, a, b = (np.asarray(r["emb%d" % i], np.float64) for i in range(3))
        return np.stack([(q * a).sum(-1), (q * b).sum(-1)], 1)

    bad, worst = [], 0.0
    for n in sorted(base):
        D = float(np.abs(np.asarray(eager[n], np.float64) - base[n]).max())
        if n == "loss":   # one scalar: its scale is what the eager tower's own logit errors can move it by (tests/test_gpu_model.py)
            D = float(np.abs(logits(eager) - logits(base)).sum(1).mean())
        d = float(np.abs(np.asarray(got[n], np.float64) - base[n]).max())
        bound = max(4.0 * D, 16.0 * A.ulp32(np.abs(base[n]).max()))
        worst = max(worst, d / bound)
        print("packed precision=half %s %-58s |half - fp32| %.3e  D %.3e  ratio %6.2f  bound %.3e%s"
              % (dt, n, d, D, d / D if D > 0 else float("nan"), bound, "" if d <= bound else "  BEYOND ITS BOUND"))
        if not d <= bound:
            bad.append((n, d, D, bound))
    print("packed precision=half %s largest d / bound %.3f" % (dt, worst))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- overflow
def _model_and_optimizer(cfg, setting, p=0.1):
    from ance_amd import model, optim
    m = _load(model.RobertaDot_NLL_LN(_config(cfg, p)), M.model_state(cfg)).train().set_packed_rows(*setting)
    named = list(m.named_parameters())
    groups = [dict(params=[q for n, q in named if S.group_of(n.replace("roberta.", "")) == k], lr=U.GROUPS[k]["lr"],
                   weight_decay=U.GROUPS[k]["weight_decay"]) for k in range(len(U.GROUPS))]
    return m, optim.Lamb(groups, lr=1e-3, betas=U.BETAS, eps=U.EPS, max_grad_norm=1.0)


def test_overflow_of_the_capacity_is_a_nan_a_count_and_a_skipped_step():
    """The body capacity one row short of the positive call (the larger body call): its last sequence is dropped -- embedding NaN, packed_dropped == 1 --
    while every other embedding stays within the bound of the full-capacity run (the same bound as against fp64: 4 x the eager fp32
    restatement's distance, floor 16 ulp).  Under a GradScaler the Lamb step then changes no parameter bit."""
    cfg = ROBERTA_BASE
    calls = S.batches(cfg, 0, 0)
    args = _call_args(calls)
    tot = [int(c["lens"].sum()) for c in calls]
    sd = M.model_state(cfg)
    masks = None
    want = M.reference_step(sd, ("roberta.",) * 3, [dict(c, types=None) for c in calls], cfg, "triplet", masks, 0.0, "float64", True)
    ref32 = M.reference_step(sd, ("roberta.",) * 3, [dict(c, types=None) for c in calls], cfg, "triplet", masks, 0.0, "float32", True)
    embs = {}
    assert tot[1] - 1 >= tot[2]   # the negative call still fits
    for name, body in (("full", tot[1]), ("short", tot[1] - 1)):
        m, _ = _model_and_optimizer(cfg, (tot[0], body), p=0.0)
        with torch.no_grad():
            embs[name] = [_np(m.query_emb(args[0], args[1])), _np(m.body_emb(args[2], args[3])), _np(m.body_emb(args[4], args[5]))]
        assert int(m.packed_dropped) == (0 if name == "full" else 1)
    assert np.isnan(embs["short"][1][-1]).all() and np.isfinite(embs["short"][1][:-1]).all()
    got = {"emb0": embs["short"][0], "emb1": embs["short"][1][:-1], "emb2": embs["short"][2]}
    full = {"emb0": embs["full"][0], "emb1": embs["full"][1][:-1], "emb2": embs["full"][2]}
    ref_err = {"emb%d" % i: float(np.abs(ref32["embs"][i].astype(np.float64) - want["embs"][i]).max()) for i in range(3)}
    bad, _ = S.compare("overflow: the kept sequences", got, full, ref_err)
    assert not bad, bad

    m, opt = _model_and_optimizer(cfg, (tot[0], tot[1] - 1))
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    before = [q.detach().clone() for q in m.parameters()]
    loss = m(*args)[0]
    assert not bool(torch.isfinite(loss))   # the NaN embedding makes the objective non-finite (nll_loss: inf or NaN)
    scaler.scale(loss).backward()
    scaler.step(opt)
    scaler.update()
    assert int(m.packed_dropped) == 1
    assert all(_bits_equal(a, b.detach()) for a, b in zip(before, m.parameters()))
    assert scaler.get_scale() < 1024.0


# ---------------------------------------------------------------------------------------------------------------- capture
def _varied_inputs(cfg, t):
    """Step t's three batches at train_step_util.SHAPES with lengths that differ from step to step: other lengths, other totals."""
    out = []
    for k, c in enumerate(S.batches(cfg, t, S.TRIPLET_SEEDS[t % len(S.TRIPLET_SEEDS)])):
        L = c["ids"].shape[1]
        lens = np.array([max(1, (int(n) * (3 + t + k)) % (L + 1)) for n in c["lens"]], np.int32)
        ids = c["ids"].copy()
        fill = S.batches(cfg, t + 7, 5)[k]["ids"]
        ids = np.where(ids == cfg["pad"], np.where(fill == cfg["pad"], 5, fill), ids)
        ids[np.arange(L)[None, :] >= lens[:, None]] = cfg["pad"]
        out.append(dict(c, ids=ids, lens=lens))
    return out


def _snapshot(m, opt):
    return [(q.detach().clone(), opt.state[q]["exp_avg"].clone(), opt.state[q]["exp_avg_sq"].clone()) for q in m.parameters()]


def test_three_replayed_packed_steps_of_different_lengths_equal_the_eager_steps():
    """RobertaDot_NLL_LN + Lamb, N = 2, dropout 0.1, int capacities: one captured step, replayed on three batches whose lengths and
    totals differ (fed by copy_), equals three eager host-mode steps with the same capacities in every parameter and both moments,
    bit for bit -- the packed row count never reaches the host."""
    from ance_amd import attention as T
    cfg, steps = ROBERTA_BASE, 3
    batches = [_varied_inputs(cfg, t) for t in range(steps)]
    totals = [[int(c["lens"].sum()) for c in b] for b in batches]
    assert len(set(map(tuple, totals))) == steps and len({tuple(map(tuple, (c["lens"] for c in b))) for b in batches}) == steps
    setting = (max(t[0] for t in totals) + 2, max(max(t[1:]) for t in totals) + 3)
    inputs = [_call_args(b) for b in batches]
    m, opt = _model_and_optimizer(cfg, setting)
    T.dropout_state.to_host(0)
    T.manual_seed(SEED)
    want = []
    for t in range(steps):
        m(*inputs[t])[0].backward()
        opt.step()
        want.append(_snapshot(m, opt))
        opt.zero_grad(set_to_none=True)
    assert int(m.packed_dropped) == 0

    m, opt = _model_and_optimizer(cfg, setting)
    T.dropout_state.to_host(0)
    T.manual_seed(SEED)
    T.dropout_state.to_device(0)
    static = [x.clone() for x in inputs[0]]
    start = [q.detach().clone() for q in m.parameters()]

    def step():
        m(*static)[0].backward()
        opt.step()
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
        for q, q0 in zip(m.parameters(), start):
            q.copy_(q0)
            st = opt.state[q]
            st["exp_avg"].zero_()
            st["exp_avg_sq"].zero_()
            if isinstance(st.get("step"), torch.Tensor):
                st["step"].zero_()
    T.manual_seed(SEED)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for t in range(steps):
        for dst, src in zip(static, inputs[t]):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        got = _snapshot(m, opt)
        for (n, _), a, b in zip(m.named_parameters(), want[t], got):
            for k, (x, y) in enumerate(zip(a, b)):
                assert _bits_equal(x, y), "step %d %s %s: max |d| %.3e" % (t, n, "pmv"[k], float((x.double() - y.double()).abs().max()))
    assert int(m.packed_dropped) == 0
    assert not _bits_equal(want[0][0][0], want[1][0][0])
