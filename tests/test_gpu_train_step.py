"""Whole training steps of the trainers' tower on the GPU -- BertEmbeddings, N x BertLayer, the head, an objective, a fused
optimizer -- several steps deep, against the fp64 restatement of tests/train_step_util.py (which tests/test_train_step.py holds to
the pieces' own NumPy oracles and to finite differences).

Teacher forcing: LAMB's and Adam's first updates are close to lr sign(g), so an element whose true gradient is rounding noise
(attention.self.key.bias is entirely such elements) gets another sign on the two sides and a free-running fp64 trajectory proves
nothing.  Every step is checked in two links instead, and the next step starts from the device's state on both sides:

  gradient link   the device's loss and gradients at the device's CURRENT parameters (read back) against tower_fp64 at those same
                  parameters, with the restated dropout masks of the offsets the step must have drawn: per tensor
                  max |got - fp64| <= max(4 x ref_err, 16 ulp32 of the fp64 tensor's largest magnitude), ref_err the eager fp32
                  composition's own distance from fp64 (attention_train_util.bound)
  update link     the device's new parameters and moments against the fp64 optimizer restatement applied to the DEVICE'S OWN
                  gradients: LAMB at tests/test_gpu_lamb_clip.py's bound for one fused clipped step against fp64 (p, m, v within
                  4 ulp32 of the tensor's largest magnitude, wn / an / tr within 2^-22 relative, last_grad_norm within 1 ulp32); AdamW
                  at adamw_util.bound (max(4 x the fp32 restatement's own distance from fp64, 2 ulp32))

The shapes cross the kernels' granularities, not the workload's: 36, 120 and 123 rows per call (no multiple of the tails' 16),
lengths 1, 17, 33 among them, ids that occur in all three calls of a step and twice in one sequence, the pad id in every batch.
Every comparison prints name, d, ref_err (or D), ratio, bound."""
import numpy as np
import pytest
import torch

import attention_train_util as A
import embeddings_util as E
import lamb_util as U
import layer_half_util as HU
import layer_tail_util as LT
import train_step_util as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = S.SEED
EMBED_BACKWARD_KERNELS = ("embed_bwd_kernel", "seg_piece_kernel", "seg_join_kernel")


def _np(t):
    return t.detach().cpu().numpy().copy()


def _dev_calls(calls):
    return [(torch.from_numpy(c["ids"]).to(DEV), None if c["types"] is None else torch.from_numpy(c["types"]).to(DEV),
             torch.from_numpy(c["lens"]).to(DEV)) for c in calls]


def _params(tower):
    return {n: _np(q) for n, q in tower.named_parameters()}


def _grads(tower):
    return {n: _np(q.grad) for n, q in tower.named_parameters() if q.grad is not None}


def _moments(tower, opt):
    return {n: (_np(opt.state[q]["exp_avg"]), _np(opt.state[q]["exp_avg_sq"])) for n, q in tower.named_parameters() if opt.state.get(q)}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _device_loss(kind, embs):
    from ance_amd.loss import biencoder_nll_loss, nll_loss
    if kind == "triplet":
        return nll_loss(*embs)
    return biencoder_nll_loss(embs[0], embs[1], torch.arange(len(embs[0]), device=DEV))[0]


def _forward_backward(tower, dcalls, kind, autocast=None, scaler=None):
    """One tower, every call of the step, one backward.  Returns the (unscaled) loss tensor."""
    with torch.autocast("cuda", dtype=autocast or torch.float16, enabled=autocast is not None):
        loss = _device_loss(kind, [tower(*c) for c in dcalls])
    (loss if scaler is None else scaler.scale(loss)).backward()
    return loss


def _word_split(grads, rows):
    """The word table's gradient as the rows that occur; the rest is returned apart (it must be exactly zero)."""
    g = dict(grads)
    rest = np.ones(len(g[S.WORD]), bool)
    rest[rows] = False
    other = g[S.WORD][rest]
    g[S.WORD] = g[S.WORD][rows]
    return g, other


def _gradient_link(tag, cfg, kind, calls, masks, p, params, loss, grads, found):
    """The device's loss and gradients at `params` against tower_fp64 at the same parameters; returns the largest d / bound and
    appends what is beyond its bound to `found` (asserted empty at the end of the test, so that every step is still measured)."""
    want = S.tower_fp64(params, calls, cfg, kind, masks, p)
    eager = S.tower_eager_fp32(params, calls, cfg, kind, masks, p)
    rows = S.occurring_rows(calls, cfg["pad"])
    assert cfg["pad"] not in rows and set(S.PLANTED) <= set(rows.tolist())
    got, other = _word_split(grads, rows)
    assert not other.any(), "the word table's gradient is not exactly zero at the rows that do not occur and at the pad row"
    w, _ = _word_split(want["grads"], rows)
    e, _ = _word_split(eager["grads"], rows)
    assert sorted(got) == sorted(w)
    got["loss"], w["loss"], e["loss"] = np.float64(loss), np.float64(want["loss"]), np.float64(eager["loss"])
    bad, worst = S.compare(tag, got, w, S.distances(e, w), ("loss",) + S.param_names(cfg))
    found.extend((tag,) + b for b in bad)
    return worst


def _lamb_link(tag, before, grads, moments, tower, opt, found):
    """The device's p, m, v, (wn, an, tr) and last_grad_norm against lamb_update_fp64 on the device's own gradients."""
    total, coef, want = S.lamb_update_fp64(before, grads, moments)
    norm = float(opt.last_grad_norm)
    print("%s: last_grad_norm %.9g (fp64 of the device's gradients %.12g), coef %.6g" % (tag, norm, total, coef))
    assert coef < 1.0 and abs(norm - total) <= U.ulp32(total), (norm, total)
    after, m_after = _params(tower), _moments(tower, opt)
    assert sorted(want) == sorted(after) == sorted(m_after)
    zero = {n: 0.0 for n in want}
    worst = 0.0
    for ix, key in enumerate(("p", "m", "v")):
        got = {n: after[n] if ix == 0 else m_after[n][ix - 1] for n in want}
        bad, w = S.compare("%s %s" % (tag, key), got, {n: want[n][ix] for n in want}, zero, floor_ulps=4.0)
        found.extend((tag, key) + b for b in bad)
        worst = max(worst, w)
    named = dict(tower.named_parameters())
    for n in want:
        st = opt.state[named[n]]
        for key, x in zip(("weight_norm", "adam_norm", "trust_ratio"), want[n][3:]):
            assert abs(float(st[key]) - x) <= 2.0 ** -22 * abs(x), (tag, n, key, float(st[key]), x)
    return worst


def _adamw_link(tag, before, grads, moments, t, tower, opt, found):
    total, coef, want = S.adamw_update_fp64(before, grads, moments, t)
    ref = S.adamw_update_fp32(before, grads, moments, t)
    norm = float(opt.last_grad_norm)
    print("%s: last_grad_norm %.9g (fp64 of the device's gradients %.12g), coef %.6g" % (tag, norm, total, coef))
    assert coef < 1.0 and abs(norm - total) <= U.ulp32(total), (norm, total)
    after, m_after = _params(tower), _moments(tower, opt)
    named = dict(tower.named_parameters())
    worst = 0.0
    for ix, key in enumerate(("p", "m", "v")):
        got = {n: after[n] if ix == 0 else m_after[n][ix - 1] for n in want}
        w64 = {n: want[n][ix] for n in want}
        bad, w = S.compare("%s %s" % (tag, key), got, w64, S.distances({n: ref[n][ix] for n in want}, w64), floor_ulps=2.0)
        found.extend((tag, key) + b for b in bad)
        worst = max(worst, w)
    assert all(float(opt.state[named[n]]["step"]) == t for n in want)
    return worst


# ------------------------------------------------------------------------------------------------------------------------ fp32, LAMB
def _triplet_run(p, check):
    """Three steps of the fp32 tower under Lamb(max_grad_norm=1.0); with `check`, both links at every step.  Returns the final
    parameters and the largest d / bound seen."""
    from ance_amd import attention as T
    from ance_amd.optim import Lamb
    cfg, kind, per_step = S.BASE, "triplet", 3 * S.draws_per_call(S.BASE)
    tower = S.device_tower(cfg, S.tower_state(cfg), 0.1)
    tower.train() if p else tower.eval()
    opt = Lamb(S.param_groups(tower), lr=1e-3, betas=U.BETAS, eps=U.EPS, max_grad_norm=1.0)
    T.manual_seed(SEED)
    worst, found = 0.0, []
    for t in range(3):
        calls = S.step_calls(cfg, kind, t)
        dcalls = _dev_calls(calls)
        before, moments = (_params(tower), _moments(tower, opt)) if check else (None, None)
        torch.cuda.synchronize()
        prev = torch.cuda.get_sync_debug_mode()
        if t == 2:   # not the first step, which allocates the optimizer's state: nothing in a whole step waits for the host
            torch.cuda.set_sync_debug_mode("error")
        try:
            loss = _forward_backward(tower, dcalls, kind)
            opt.step()
        finally:
            torch.cuda.set_sync_debug_mode(prev)
        assert T.dropout_state.offsets.get(0, 0) == ((t + 1) * per_step if p else 0)
        if check:
            tag = "triplet p %.1f step %d" % (p, t)
            grads = _grads(tower)
            masks = S.calls_masks(p, SEED, t * per_step, cfg, calls)
            worst = max(worst, _gradient_link(tag, cfg, kind, calls, masks, p, before, float(loss.detach()), grads, found))
            worst = max(worst, _lamb_link(tag, before, grads, moments, tower, opt, found))
        opt.zero_grad(set_to_none=True)
    return _params(tower), worst, found


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_triplet_step_fp32_lamb(p):
    """Query, positive and negative through ONE tower (H 768, 2 layers, absolute positions, 2 token types), nll_loss on the three
    first-token rows, one backward, Lamb(max_grad_norm=1.0) with lamb_util.GROUPS' two groups; three steps, zero_grad(set_to_none)
    between them.  Both links at every step; the word table's gradient exactly zero at the rows that do not occur and at the pad
    row; with p = 0.1 the dropout counter stands at (t + 1) 3 (1 + 3 N) after step t and the reference's masks are step_masks at
    those offsets, with p = 0 the tower is in eval() and the counter stays 0; step 3 runs under set_sync_debug_mode("error"); the
    whole run repeated after manual_seed gives the same bits in every parameter.
    What this test found: attention.self.key.bias has no gradient at all (a softmax does not see a constant added to a row of
    scores), the fp64 tensor is 1e-16, and BertLayer handed back the rounding noise of the column sum of dk there: 1.4e-07 and
    2.2e-07 for layer 0 at step 0, 4.1 and 5.0 x the eager composition's own noise and beyond this rule, which has no floor at a
    tensor of zeros.  BertLayer now gives that parameter a gradient of exact zeros.
    Measured: 0.62 of the bound at most with p 0 and 0.76 with p 0.1, both links over the three steps."""
    params, worst, found = _triplet_run(p, True)
    print("triplet p %.1f: largest d / bound over three steps %.2f" % (p, worst))
    again, _, _ = _triplet_run(p, False)
    for n in params:
        assert np.array_equal(_bits(params[n]), _bits(again[n])), n
    assert not found, found


# ------------------------------------------------------------------------------------------------------------------------ H 1024, AdamW
def test_inbatch_step_large_adamw():
    """H 1024, 16 heads, one layer, RoBERTa positions, one token type, eps 1e-12: biencoder_nll_loss of 3 queries against ONE context
    call of 6 sequences (positives at 0, 1, 2), AdamW(max_grad_norm=1.0), two steps, dropout 0.1.  Both links at every step.
    What this test found, both in the in-batch objective's kernels and both visible only at the scores of LayerNorm outputs (600 -
    900 here): (1) lse = max + log(sum) was kept as ONE float and softmax formed as exp(s - lse); lse is only known to ulp(900) =
    6e-5 there, which became a RELATIVE error of every gradient of the step, 17 - 106 x ref_err.  The kernels now keep the two terms
    apart, exp((s - max) - log sum).  (2) The scores' 64 k-tile sums were added in fp32, 1e-4 at that magnitude; step 1's loss is
    not saturated, its softmax sees that, and attention.self.key.weight stood at 1.02 of its bound (4.1 x ref_err).  The tiles are
    now summed in fp64 and rounded once.
    Measured: 0.52 of the bound at most, both links over the two steps."""
    from ance_amd import attention as T
    from ance_amd.optim import AdamW
    cfg, kind, p = S.LARGE, "inbatch", 0.1
    per_step = 2 * S.draws_per_call(cfg)
    tower = S.device_tower(cfg, S.tower_state(cfg), p).train()
    opt = AdamW(S.param_groups(tower), lr=1e-3, betas=U.BETAS, eps=U.EPS, max_grad_norm=1.0)
    T.manual_seed(SEED)
    worst, found = 0.0, []
    for t in range(2):
        calls = S.step_calls(cfg, kind, t)
        before, moments = _params(tower), _moments(tower, opt)
        loss = _forward_backward(tower, _dev_calls(calls), kind)
        opt.step()
        assert T.dropout_state.offsets.get(0, 0) == (t + 1) * per_step
        tag, grads = "inbatch step %d" % t, _grads(tower)
        masks = S.calls_masks(p, SEED, t * per_step, cfg, calls)
        worst = max(worst, _gradient_link(tag, cfg, kind, calls, masks, p, before, float(loss.detach()), grads, found))
        worst = max(worst, _adamw_link(tag, before, grads, moments, t + 1, tower, opt, found))
        opt.zero_grad(set_to_none=True)
    print("inbatch: largest d / bound over two steps %.2f" % worst)
    assert not found, found


# ------------------------------------------------------------------------------------------------------------------------ frozen
def _traced_kernels(fn):
    """Names of the kernels of one call, from torch.profiler (as tests/test_gpu_embeddings.py)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events()
            if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]


def test_frozen_embeddings_and_layernorms():
    """embeddings.* and every LayerNorm.* with requires_grad off, one forward / backward of the triplet step at dropout 0.1: the
    frozen parameters keep grad None, every other gradient has the bits of the unfrozen run from the same seed (an on-device
    comparison: the unfrozen run is the one test_triplet_step_fp32_lamb[0.1] holds to fp64 at step 0, same inputs), the embedding
    backward's kernels are not launched and the backward launches fewer kernels than the unfrozen one (measured: 243 launches
    against 320, 9 of those the embedding backward's)."""
    from ance_amd import attention as T
    cfg, kind = S.BASE, "triplet"
    dcalls = _dev_calls(S.step_calls(cfg, kind, 0))
    runs = {}
    for frozen in (False, True):
        tower = S.device_tower(cfg, S.tower_state(cfg), 0.1).train()
        cold = [n for n, _ in tower.named_parameters() if frozen and (n.startswith("embeddings.") or ".LayerNorm." in n)]
        for n, q in tower.named_parameters():
            q.requires_grad_(n not in cold)
        T.manual_seed(SEED)
        with torch.no_grad():   # the profiler's first use and the kernels' first launches stay out of the traced backward
            tower(*dcalls[0])
        T.manual_seed(SEED)
        loss = _device_loss(kind, [tower(*c) for c in dcalls])
        kernels = _traced_kernels(loss.backward)
        runs[frozen] = (_grads(tower), kernels, cold)
        for n, q in tower.named_parameters():
            assert (q.grad is None) == (n in cold), n
    (full, k_full, _), (part, k_part, cold) = runs[False], runs[True]
    assert len(cold) == 5 + 4 * cfg["N"] and sorted(part) == sorted(set(full) - set(cold))
    for n in part:
        assert np.array_equal(_bits(part[n]), _bits(full[n])), n
    ours = lambda names: [n for n in names if any(k in n for k in EMBED_BACKWARD_KERNELS)]   # noqa: E731
    print("backward launches: %d unfrozen (%d of the embedding backward), %d frozen" % (len(k_full), len(ours(k_full)), len(k_part)))
    assert len(ours(k_full)) == 3 * len(EMBED_BACKWARD_KERNELS), ours(k_full)   # three tower calls
    assert ours(k_part) == [], ours(k_part)
    assert len(k_part) < len(k_full), (len(k_part), len(k_full))


# ------------------------------------------------------------------------------------------------------------------------ the --fp16 recipe
def _eager_autocast_grads(params, calls, cfg, kind, dtype, scale):
    """torch's own embeddings, layer_half_util.eager_layer chained and torch's head under torch.autocast on the device, the loss
    scaled as the recipe scales it: {name: unscaled gradient, "loss": the loss}."""
    F = torch.nn.functional
    Wt = {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in params.items()}
    with torch.autocast("cuda", dtype=dtype):
        embs = []
        for c in calls:
            h = E.embed_torch_forward(c["ids"], c["types"], *(Wt[n] for n in S.EMB), cfg["eps"], cfg["mode"], cfg["pad"])
            rows = torch.from_numpy(A._valid(c["lens"], c["ids"].shape[1])).to(DEV)
            for i in range(cfg["N"]):
                pre = S.layer_prefix(i)
                h = HU.eager_layer(h.float(), rows, {n: Wt[pre + n] for n in LT.LAYER_PARAMS}, cfg["heads"], cfg["eps"])
            e = F.linear(h[:, 0].contiguous(), Wt["embeddingHead.weight"], Wt["embeddingHead.bias"])
            embs.append(F.layer_norm(e, (cfg["H"],), Wt["norm.weight"], Wt["norm.bias"], S.HEAD_EPS).float())
        loss = S.loss_torch(kind, embs)
    (loss * scale).backward()
    return dict({k: _np(w.grad) / np.float32(scale) for k, w in Wt.items()}, loss=np.float32(float(loss.detach())))


@pytest.mark.parametrize("dt", HU.DTYPES)
def test_fp16_recipe_step(dt):
    """The --fp16 recipe end to end: the triplet tower with BertLayer(precision="half") chained through the 16-bit copy
    (return_half / hidden_states_half), fp32 embeddings, torch.autocast, dropout 0, Lamb(max_grad_norm=1.0); for fp16 a
    torch.amp.GradScaler(init_scale=2^10) drives the step through scaler.step.  Two steps, each in two links:
      gradient link  per tensor |half tower - fp32 tower on the device| <= max(4 D, 16 ulp32), D the distance of the eager autocast
                     composition from the same fp32 device tower, all three at the device's current parameters, gradients unscaled
                     by the exact power of two.  The fp32 device tower is admissible as the base ONLY because
                     test_triplet_step_fp32_lamb[0.0] holds it to fp64 on the same inputs;
      update link    the fp64 LAMB restatement on the device's unscaled gradients (4 ulp32; the norm 1 ulp32).
    Then, for fp16, one overflow step: the scale is set to the smallest 2^k at which the fp64 reference's largest 16-bit activation
    gradient, scaled, exceeds 4 x 65504 (computed here, asserted <= 2^40); after scaler.step / scaler.update no bit of any
    parameter or moment has changed, skipped_steps is 1 and the scale has halved.  At the halved scale that gradient still exceeds
    2 x 65504, so the following step, which passes both links again, runs after the scale is set back to 2^10.
    The loss is one number per step, and so is D for it: it is held to 4 x the largest D of the run's steps.
    Measured: 0.41 of the bound at most for fp16 and 0.58 for bf16 (both links and the loss);
    the reference's largest 16-bit activation gradient is 1.39, the overflow scale 2^18."""
    from ance_amd.optim import Lamb
    cfg, kind, dtype = S.BASE, "triplet", HU.torch_dtype(dt)
    half = S.device_tower(cfg, S.tower_state(cfg), 0.0, "half").train()
    base = S.device_tower(cfg, S.tower_state(cfg), 0.0).train()
    opt = Lamb(S.param_groups(half), lr=1e-3, betas=U.BETAS, eps=U.EPS, max_grad_norm=1.0)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10) if dt == "fp16" else None
    worst, found, losses = 0.0, [], []

    def step(t):
        calls = S.step_calls(cfg, kind, t)
        dcalls = _dev_calls(calls)
        before, moments = _params(half), _moments(half, opt)
        scale = scaler.get_scale() if scaler is not None else 1.0
        loss = _forward_backward(half, dcalls, kind, dtype, scaler)
        scaled = _grads(half)
        if scaler is None:
            opt.step()
        else:
            scaler.step(opt)
            scaler.update()
        opt.zero_grad(set_to_none=True)
        return calls, dcalls, before, moments, scale, float(loss.detach()), scaled

    def links(tag, calls, dcalls, before, moments, scale, loss, scaled):
        grads = {n: g / np.float32(scale) for n, g in scaled.items()}   # a power of two: exact
        base.load_state_dict({k: torch.from_numpy(v) for k, v in before.items()}, strict=True)
        base.zero_grad(set_to_none=True)
        base_loss = float(_forward_backward(base, dcalls, kind))
        want = dict(_grads(base), loss=np.float32(base_loss))
        eager = _eager_autocast_grads(before, calls, cfg, kind, dtype, scale)
        D = S.distances(eager, want, ("loss",) + S.param_names(cfg))
        losses.append((tag, abs(loss - base_loss), D["loss"], 16.0 * A.ulp32(base_loss)))
        bad, w1 = S.compare(tag + " " + dt, grads, want, D, S.param_names(cfg))
        found.extend((tag,) + b for b in bad)
        return max(w1, _lamb_link(tag + " " + dt, before, grads, moments, half, opt, found))

    for t in range(2):
        tag = "half step %d" % t
        r = step(t)
        assert r[4] == (2.0 ** 10 if scaler is not None else 1.0)
        worst = max(worst, links(tag, *r))
    if scaler is not None:
        assert int(opt.skipped_steps) == 0
        # the overflow step: the scale from the fp64 reference's 16-bit activation gradients at the device's parameters
        calls, taps = S.step_calls(cfg, kind, 2), []
        S.tower_fp64(_params(half), calls, cfg, kind, taps=taps)
        largest = max(float(x.grad.abs().max()) for _, x in taps)
        k = int(np.floor(np.log2(4 * 65504.0 / largest))) + 1
        assert largest * 2.0 ** k > 4 * 65504.0 >= largest * 2.0 ** (k - 1) and k <= 40, (largest, k)
        print("overflow step: the reference's largest 16-bit activation gradient %.3e, scale 2^%d" % (largest, k))
        scaler.update(new_scale=2.0 ** k)
        before, moments = _params(half), _moments(half, opt)
        r = step(2)
        assert r[4] == 2.0 ** k
        after, m_after = _params(half), _moments(half, opt)
        for n in before:
            assert np.array_equal(_bits(before[n]), _bits(after[n])), n
            for a, b in zip(moments[n], m_after[n]):
                assert np.array_equal(_bits(a), _bits(b)), n
        assert int(opt.skipped_steps) == 1 and scaler.get_scale() == 2.0 ** (k - 1)
        assert not all(np.isfinite(g).all() for g in r[6].values())
        scaler.update(new_scale=2.0 ** 10)
        r = step(2)
        assert r[4] == 2.0 ** 10
        worst = max(worst, links("half step after the overflow", *r))
        assert int(opt.skipped_steps) == 1
    # the loss is ONE number per step, and so is the eager composition's distance: a single draw, not a maximum over a tensor's
    # elements.  Its D is therefore the largest of the run's steps (still the references' figures alone).
    D_loss = max(D for _, _, D, _ in losses)
    for tag, d, D, floor in losses:
        print("%-28s %-58s d %.3e  D %.3e  D of the run %.3e  bound %.3e" % (tag + " " + dt, "loss", d, D, D_loss, max(4 * D_loss, floor)))
        if not d <= max(4 * D_loss, floor):
            found.append((tag, "loss", d, D_loss))
        worst = max(worst, d / max(4 * D_loss, floor))
    print("half %s: largest d / bound %.2f" % (dt, worst))
    assert not found, found
