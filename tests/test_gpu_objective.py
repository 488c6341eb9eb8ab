"""The objectives with gradients (ance_amd/loss.py -> csrc/nll.hip, csrc/inbatch_nll.hip) on the GPU against the fp64 restatement
(tests/objective_util.py) and the reference's own gradients (tests/golden/objective.*).

Bound, per tensor: max(4 x the reference's own max |delta| from fp64, 2 ulp of the tensor's largest magnitude) -- the form of
tests/test_gpu_lamb.py.  The reference's distance is the one recorded in the golden for that case; for the seeded cases without a
golden it is that of the same torch fp32 expression evaluated here on the CPU.  Every measured distance is printed."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import objective_util as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _golden(golden_dir):
    with open(os.path.join(golden_dir, "objective.json")) as f:
        return json.load(f), np.load(os.path.join(golden_dir, "objective.npz"))


def _dev(x, grad=True):
    if x is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t.requires_grad_(True) if grad else t


def _np64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _check_loss(tag, got, want, ref, largest_logit):
    """The loss moves by at most the error of the logits it is made of (|d loss / d logit| <= 1), and an fp32 dot product is within
    a few ulp of its own magnitude: max(4 x the reference's distance, 4 ulp of the largest |logit|)."""
    got, ref = (float(x.detach()) if isinstance(x, torch.Tensor) else float(x) for x in (got, ref))
    d, b = abs(got - want), max(4 * abs(float(ref) - want), 4 * O.U.ulp32(largest_logit))
    print("%-28s |delta| %.3e  reference %.3e  bound %.3e" % (tag + " loss", d, abs(float(ref) - want), b))
    assert d <= b, (tag, d, b)


def _check(tag, got, want, ref_err):
    d = float(np.abs(_np64(got) - want).max())
    b = O.bound(ref_err, np.abs(want).max())
    print("%-28s max|delta| %.3e  reference %.3e  bound %.3e" % (tag, d, ref_err, b))
    assert d <= b, (tag, d, b)


def _torch_triplet(q, a, b, ma, mb, go=1.0):
    """The reference's expression (model/models.py:77-81, 109-134) in torch fp32 on the CPU: loss and gradients."""
    tq, ta, tb = (torch.from_numpy(np.array(x)).requires_grad_(True) for x in (q, a, b))
    if a.ndim == 2:
        la, lb = (tq * ta).sum(-1), (tq * tb).sum(-1)
    else:
        la = (torch.matmul(tq.unsqueeze(1), ta.transpose(1, 2))[:, 0, :] + (1 - torch.from_numpy(ma)) * -9999).max(dim=-1).values
        lb = (torch.matmul(tq.unsqueeze(1), tb.transpose(1, 2))[:, 0, :] + (1 - torch.from_numpy(mb)) * -9999).max(dim=-1).values
    loss = (-1.0 * F.log_softmax(torch.cat([la.unsqueeze(1), lb.unsqueeze(1)], dim=1), dim=1)[:, 0]).mean()
    (go * loss).backward()
    return loss, tq.grad, ta.grad, tb.grad


def _torch_inbatch(q, ctx, pos):
    tq, tc = (torch.from_numpy(np.array(x)).requires_grad_(True) for x in (q, ctx))
    loss = F.nll_loss(F.log_softmax(torch.matmul(tq, tc.t()), dim=1), torch.from_numpy(pos), reduction="mean")
    loss.backward()
    return loss, tq.grad, tc.grad


def _run_triplet(q, a, b, ma, mb, factor=None):
    from ance_amd.loss import nll_loss
    tq, ta, tb = _dev(q), _dev(a), _dev(b)
    loss = nll_loss(tq, ta, tb, _dev(ma, False), _dev(mb, False))
    assert loss.dim() == 0 and loss.grad_fn is not None
    (loss if factor is None else factor * loss).backward()
    return loss, tq.grad, ta.grad, tb.grad


def test_forward_is_bit_identical_to_ance_nll_forward():
    from ance_amd import _lib
    from ance_amd.loss import nll_loss
    for case in ("firstp_n64", "maxp"):
        q, a, b, ma, mb = O.triplet_inputs(case)
        tq, ta, tb, tma, tmb = _dev(q, False), _dev(a, False), _dev(b, False), _dev(ma, False), _dev(mb, False)
        n, d = q.shape
        chunks = 1 if a.ndim == 2 else a.shape[1]
        lg, rw, mn = torch.empty((n, 2), device=DEV), torch.empty(n, device=DEV), torch.empty(1, device=DEV)
        P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        _lib.check(_lib.lib().ance_nll_forward(P(tq), P(ta), P(tb), P(tma), P(tmb), n, d, chunks, P(lg), P(rw), P(mn),
                                               _lib.current_stream_ptr()), "ance_nll_forward")
        loss, logits, rows = nll_loss(tq.requires_grad_(True), ta, tb, tma, tmb, return_rows=True)
        np.testing.assert_array_equal(loss.detach().cpu().numpy(), mn[0].cpu().numpy())
        np.testing.assert_array_equal(logits.cpu().numpy(), lg.cpu().numpy())
        np.testing.assert_array_equal(rows.cpu().numpy(), rw.cpu().numpy())
        assert not logits.requires_grad and not rows.requires_grad


@pytest.mark.parametrize("case", list(O.FIRSTP_CASES) + list(O.DPR_TRIPLET_CASES) + ["maxp"])
def test_triplet_gradients_on_the_golden_inputs(golden_dir, case):
    j, g = _golden(golden_dir)
    q, a, b, ma, mb = O.triplet_inputs(case)
    want = O.nll_fp64(q, a, b, ma, mb)
    loss, gq, ga, gb = _run_triplet(q, a, b, ma, mb)
    _check_loss(case, loss, want["loss"], j[case]["loss"], np.abs(want["logits"]).max())
    for k, got in (("gq", gq), ("ga", ga), ("gb", gb)):
        _check("%s.%s" % (case, k), got, want[k], j[case]["ref_err"][k])
        # and the reference's own fp32 gradient, on the elements the golden keeps
        d = np.abs(O.recorded(_np64(got)) - g["%s.%s" % (case, k)]).max()
        assert d <= O.bound(j[case]["ref_err"][k], np.abs(want[k]).max()) + j[case]["ref_err"][k]


def test_maxp_losing_and_masked_chunk_rows_are_exact_zeros_in_nan_filled_buffers():
    from ance_amd import _lib
    q, a, b, ma, mb = O.triplet_inputs("maxp")
    want = O.nll_fp64(q, a, b, ma, mb)
    tq, ta, tb, tma, tmb = (_dev(x, False) for x in (q, a, b, ma, mb))
    go = torch.ones(1, device=DEV)
    gq, ga, gb = (torch.full_like(t, float("nan")) for t in (tq, ta, tb))
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    _lib.check(_lib.lib().ance_nll_backward(P(tq), P(ta), P(tb), P(tma), P(tmb), O.MAXP_N, O.D, O.MAXP_CHUNKS, P(go), P(gq), P(ga), P(gb),
                                            _lib.current_stream_ptr()), "ance_nll_backward")
    assert not torch.isnan(gq).any()
    for got, win, mask in ((ga.cpu().numpy(), want["ca"], ma), (gb.cpu().numpy(), want["cb"], mb)):
        for r in range(O.MAXP_N):
            assert mask[r, win[r]] == 1
            for c in range(O.MAXP_CHUNKS):
                if c == win[r]:
                    assert np.abs(got[r, c]).max() > 0
                else:
                    assert np.array_equal(got[r, c], np.zeros(O.D, np.float32)), (r, c)
    # the exact ties went to the lower index
    for name, got in (("a", ga), ("b", gb)):
        r, c0, c1 = O.MAXP_DUP[name]
        assert float(got[r, c0].abs().max()) > 0 and float(got[r, c1].abs().max()) == 0


@pytest.mark.parametrize("chunks", [1, 4])
def test_triplet_gradients_seeded_n1000(chunks):
    q, a, b, ma, mb = O.seeded_triplets(1000, chunks)
    want = O.nll_fp64(q, a, b, ma, mb)
    _, rq, ra, rb = _torch_triplet(q, a, b, ma, mb)
    loss, gq, ga, gb = _run_triplet(q, a, b, ma, mb)
    for k, got, ref in (("gq", gq, rq), ("ga", ga, ra), ("gb", gb, rb)):
        _check("seeded n=1000 chunks=%d %s" % (chunks, k), got, want[k], np.abs(ref.numpy().astype(np.float64) - want[k]).max())


def test_grad_output_scales_by_the_fp32_product_rule():
    """(3 * loss).backward(): s = 3 / n enters once, as in the restatement with grad_output = 3."""
    q, a, b, ma, mb = O.triplet_inputs("maxp")
    want = O.nll_fp64(q, a, b, ma, mb, grad_output=3.0)
    _, rq, ra, rb = _torch_triplet(q, a, b, ma, mb, go=3.0)
    _, gq, ga, gb = _run_triplet(q, a, b, ma, mb, factor=3)
    for k, got, ref in (("gq", gq, rq), ("ga", ga, ra), ("gb", gb, rb)):
        _check("3 x loss maxp %s" % k, got, want[k], np.abs(ref.numpy().astype(np.float64) - want[k]).max())
    from ance_amd.loss import biencoder_nll_loss
    q, ctx, pos = O.inbatch_inputs(7)
    want = O.inbatch_fp64(q, ctx, pos, grad_output=3.0)
    tq, tc = _dev(q), _dev(ctx)
    loss, _ = biencoder_nll_loss(tq, tc, _dev(pos, False))
    (3 * loss).backward()
    rq = torch.from_numpy(np.array(q)).requires_grad_(True)
    rc = torch.from_numpy(np.array(ctx)).requires_grad_(True)
    (3 * F.nll_loss(F.log_softmax(rq @ rc.t(), dim=1), torch.from_numpy(pos))).backward()
    _check("3 x loss inbatch gq", tq.grad, want["gq"], np.abs(rq.grad.numpy().astype(np.float64) - want["gq"]).max())
    _check("3 x loss inbatch gctx", tc.grad, want["gctx"], np.abs(rc.grad.numpy().astype(np.float64) - want["gctx"]).max())


@pytest.mark.parametrize("case", list(O.INBATCH_CASES))
def test_inbatch_on_the_golden_inputs(golden_dir, case):
    from ance_amd.loss import biencoder_nll_loss
    j, g = _golden(golden_dir)
    q, ctx, pos = O.inbatch_inputs(O.INBATCH_CASES[case])
    want = O.inbatch_fp64(q, ctx, pos)
    tq, tc = _dev(q), _dev(ctx)
    loss, n_correct, n_invalid = biencoder_nll_loss(tq, tc, _dev(pos, False), return_invalid=True)
    assert loss.dim() == 0 and loss.grad_fn is not None
    assert n_correct.dim() == 0 and n_correct.dtype == torch.int64 and n_correct.is_cuda and not n_correct.requires_grad
    loss.backward()
    _check_loss(case, loss, want["loss"], j[case]["loss"], np.abs(want["scores"]).max())
    assert int(n_correct) == want["n_correct"] == int(g[case + ".correct"].sum()) and int(n_invalid) == 0
    _check(case + ".gq", tq.grad, want["gq"], j[case]["ref_err"]["gq"])
    _check(case + ".gctx", tc.grad, want["gctx"], j[case]["ref_err"]["gctx"])


def test_inbatch_1024_by_2048_every_row_counts_and_gradients():
    """The envelope's corner (d = 768).  Every positive is planted with a margin verified in fp64 to be above 1e-3; rows 3 and 5
    carry the exact duplicates (lowest-index rule).  n_correct is compared as a total and then ROW BY ROW: each query alone
    against all 2048 passages must give that row's own verdict, so no row is skipped."""
    from ance_amd.loss import biencoder_nll_loss
    q, ctx, pos = O.inbatch_inputs(1024, d=768)
    assert O.inbatch_margins(q, ctx, pos).min() > 1e-3
    want = O.inbatch_fp64(q, ctx, pos)
    hi, lo = O.INBATCH_DUP_ROWS
    assert want["correct"][hi] and not want["correct"][lo]
    tq, tc, tp = _dev(q), _dev(ctx), _dev(pos, False)
    loss, n_correct = biencoder_nll_loss(tq, tc, tp)
    loss.backward()
    assert int(n_correct) == want["n_correct"]
    # row by row: a single query against all 2048 passages must give that row's own verdict (no row skipped)
    with torch.no_grad():
        for i in range(1024):
            _, c = biencoder_nll_loss(tq[i:i + 1].detach(), tc.detach(), tp[i:i + 1])
            assert int(c) == int(want["correct"][i]), i
    rloss, rq, rc = _torch_inbatch(q, ctx, pos)
    _check_loss("inbatch 1024x2048", loss, want["loss"], rloss, np.abs(want["scores"]).max())
    _check("inbatch 1024x2048 gq", tq.grad, want["gq"], np.abs(rq.numpy().astype(np.float64) - want["gq"]).max())
    _check("inbatch 1024x2048 gctx", tc.grad, want["gctx"], np.abs(rc.numpy().astype(np.float64) - want["gctx"]).max())


def test_inbatch_out_of_range_positive_is_counted_and_poisons_without_touching_memory():
    from ance_amd.loss import biencoder_nll_loss
    q, ctx, pos = O.inbatch_inputs(7)
    pos = pos.copy()
    pos[2], pos[4] = 14, -1
    tq, tc = _dev(q), _dev(ctx)
    loss, n_correct, n_invalid = biencoder_nll_loss(tq, tc, _dev(pos, False), return_invalid=True)
    loss.backward()
    assert int(n_invalid) == 2 and torch.isnan(loss).item() and int(n_correct) <= 5
    assert torch.isnan(tq.grad[2]).all() and torch.isnan(tq.grad[4]).all() and not torch.isnan(tq.grad[[0, 1, 3, 5, 6]]).any()


def test_autograd_through_a_linear_tower():
    """q, a, b from a small torch.nn.Linear tower on the GPU: the tower's weight.grad through nll_loss against the same graph built
    from the torch expression (fp64 on the CPU as the oracle, fp32 on the CPU as the reference's distance)."""
    from ance_amd.loss import nll_loss
    x = {k: O.det_normal(41, "obj.tower." + k, (32, 64), 1.0) for k in "qab"}
    w0, b0 = O.det_normal(41, "obj.tower.w", (128, 64), 0.05), O.det_normal(41, "obj.tower.bias", (128,), 0.05)

    def tower(dtype, device):
        lin = torch.nn.Linear(64, 128).to(device=device, dtype=dtype)
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w0))
            lin.bias.copy_(torch.from_numpy(b0))
        return lin, [lin(torch.from_numpy(x[k]).to(device=device, dtype=dtype)) for k in "qab"]

    lin, (q, a, b) = tower(torch.float32, DEV)
    nll_loss(q.contiguous(), a.contiguous(), b.contiguous()).backward()
    grads = {}
    for dtype in (torch.float64, torch.float32):
        l2, (q2, a2, b2) = tower(dtype, "cpu")
        lg = torch.cat([(q2 * a2).sum(-1).unsqueeze(1), (q2 * b2).sum(-1).unsqueeze(1)], dim=1)
        (-1.0 * F.log_softmax(lg, dim=1)[:, 0]).mean().backward()
        grads[dtype] = (l2.weight.grad.numpy().astype(np.float64), l2.bias.grad.numpy().astype(np.float64))
    for i, name in enumerate(("weight", "bias")):
        want, ref = grads[torch.float64][i], grads[torch.float32][i]
        _check("tower %s.grad" % name, getattr(lin, name).grad, want, np.abs(ref - want).max())


def test_detached_rows_concatenated_with_live_rows():
    """The DDP form (run_ann_dpr.py:340-354): this rank's rows with grad, the other ranks' detached; torch.cat's backward drops
    what is detached, the live rows get the gradient of their rows."""
    from ance_amd.loss import biencoder_nll_loss
    q, ctx, pos = O.inbatch_inputs(7)
    want = O.inbatch_fp64(q, ctx, pos)
    _, rq, rc = _torch_inbatch(q, ctx, pos)
    lq, lc = _dev(q[:4]), _dev(ctx[:8])
    oq, oc = _dev(q[4:]).detach(), _dev(ctx[8:]).detach()
    loss, _ = biencoder_nll_loss(torch.cat([lq, oq], dim=0), torch.cat([lc, oc], dim=0), _dev(pos, False))
    loss.backward()
    assert oq.grad is None and oc.grad is None
    _check("ddp live q rows", lq.grad, want["gq"][:4], np.abs(rq.numpy().astype(np.float64) - want["gq"]).max())
    _check("ddp live ctx rows", lc.grad, want["gctx"][:8], np.abs(rc.numpy().astype(np.float64) - want["gctx"]).max())


def test_no_host_wait_graph_capture_and_determinism():
    """Forward + backward of both objectives captured in one graph (a single chain on one stream; a capture raises on any host
    wait) and replayed once: the replay's bits equal an eager run's, and two eager runs agree bit for bit."""
    from ance_amd.loss import biencoder_nll_loss, nll_loss
    q, a, b, ma, mb = O.triplet_inputs("maxp")
    iq, ic, ip = O.inbatch_inputs(128)
    T = [_dev(x, False) for x in (q, a, b, ma, mb, iq, ic, ip)]

    def step():
        tq, ta, tb = (t.clone().requires_grad_(True) for t in T[:3])
        xq, xc = (t.clone().requires_grad_(True) for t in T[5:7])
        l1 = nll_loss(tq, ta, tb, T[3], T[4])
        l2, nc = biencoder_nll_loss(xq, xc, T[7])
        (2 * l1 + l2).backward()
        return [l1.detach(), l2.detach(), nc, tq.grad, ta.grad, tb.grad, xq.grad, xc.grad]

    e1 = [t.clone() for t in step()]
    e2 = [t.clone() for t in step()]
    torch.cuda.synchronize()
    for x, y in zip(e1, e2):
        assert torch.equal(x, y)
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")  # any synchronising torch call raises
    try:
        step()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()  # warm-up on the side stream, as torch's capture recipe asks
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        outs = step()
    for t in outs:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(e1, outs):
        assert torch.equal(x, y)


def test_second_derivative_raises():
    """Differentiable once.  With a constant upstream gradient, autograd gives the first derivative no grad_fn under
    create_graph, so differentiating it again raises; with an upstream gradient that itself requires grad, the
    once_differentiable guard raises by name."""
    from ance_amd.loss import nll_loss
    q, a, b, _, _ = O.triplet_inputs("firstp_n3")
    tq, ta, tb = _dev(q), _dev(a), _dev(b)
    (gq,) = torch.autograd.grad(nll_loss(tq, ta, tb), tq, create_graph=True)
    assert gq.grad_fn is None and not gq.requires_grad
    with pytest.raises(RuntimeError, match="does not require grad"):
        gq.sum().backward()
    w = torch.ones((), device=DEV, requires_grad=True)
    (gq2,) = torch.autograd.grad(w * nll_loss(tq, ta, tb), tq, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gq2.sum().backward()
