"""The trainers' objectives with gradients: where ``grad_output`` enters the library.

``nll_loss``            the triplet objective of NLL.forward / NLL_MultiChunk.forward (model/models.py:57-81, 84-134) and of the DPR
                        triplet form (:260-271): forward ``ance_nll_forward`` (the bits of ``AnceModel.forward``), backward
                        ``ance_nll_backward`` (csrc/nll.hip)
``biencoder_nll_loss``  in-batch negatives of the DPR trainer (drivers/run_ann_dpr.py:356-365, also its evaluate_dev):
                        ``ance_inbatch_nll_forward`` / ``ance_inbatch_nll_backward`` (csrc/inbatch_nll.hip)

Both are ``torch.autograd.Function``s, differentiable once.  No CPU fallback: every input is a contiguous fp32 tensor on one HIP
device.  Nothing waits for the host in forward or backward: the upstream gradient reaches the kernels as a device pointer, so a
step can be captured in a graph.  No atomics: the same inputs give the same bits.
"""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _checked(t, what, device, dtype=torch.float32):
    _lib.require_cuda_tensor(t, dtype, what)
    if device is not None and t.device != device:
        raise _lib.AnceLibraryError("%s is on %s, the other tensors of this call on %s (mixed devices)" % (what, t.device, device))
    return t


def _grad_output(g, device):
    """The upstream gradient as a contiguous fp32 device scalar (autograd may hand over an expanded view)."""
    return g.to(device=device, dtype=torch.float32).reshape(1).contiguous()


class _TripletNLL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, a, b, mask_a, mask_b):
        fn = "nll_loss"
        _checked(q, fn + ": q", None)
        if q.dim() != 2:
            raise _lib.AnceLibraryError("%s: q must be [n, d], got %s" % (fn, tuple(q.shape)))
        n, d = q.shape
        _checked(a, fn + ": a", q.device)
        _checked(b, fn + ": b", q.device)
        if a.dim() == 2:
            chunks = 1
        elif a.dim() == 3:
            chunks = a.shape[1]
        else:
            raise _lib.AnceLibraryError("%s: a must be [n, d] or [n, chunks, d], got %s" % (fn, tuple(a.shape)))
        want = (n, d) if a.dim() == 2 else (n, chunks, d)
        for name, t in (("a", a), ("b", b)):
            if tuple(t.shape) != want:
                raise _lib.AnceLibraryError("%s: %s has shape %s, expected %s" % (fn, name, tuple(t.shape), want))
        if a.dim() == 3:
            for name, m in (("mask_a", mask_a), ("mask_b", mask_b)):
                if m is None:
                    raise _lib.AnceLibraryError("%s: %s is required with [n, chunks, d] passages" % (fn, name))
                _checked(m, fn + ": " + name, q.device)
                if tuple(m.shape) != (n, chunks):
                    raise _lib.AnceLibraryError("%s: %s has shape %s, expected %s" % (fn, name, tuple(m.shape), (n, chunks)))
        else:
            mask_a = mask_b = None
        logits = torch.empty((n, 2), dtype=torch.float32, device=q.device)
        rows = torch.empty((n,), dtype=torch.float32, device=q.device)
        mean = torch.empty((1,), dtype=torch.float32, device=q.device)
        with torch.cuda.device(q.device):
            rc = _lib.lib().ance_nll_forward(_P(q), _P(a), _P(b), _P(mask_a), _P(mask_b), n, d, chunks, _P(logits), _P(rows), _P(mean),
                                             _lib.current_stream_ptr())
        _lib.check(rc, "ance_nll_forward")
        ctx.save_for_backward(q, a, b, mask_a, mask_b)
        ctx.chunks = chunks
        ctx.mark_non_differentiable(logits, rows)
        return mean[0], logits, rows

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, _grad_logits, _grad_rows):
        q, a, b, mask_a, mask_b = ctx.saved_tensors
        n, d = q.shape
        go = _grad_output(grad_loss, q.device)
        gq, ga, gb = torch.empty_like(q), torch.empty_like(a), torch.empty_like(b)
        with torch.cuda.device(q.device):
            rc = _lib.lib().ance_nll_backward(_P(q), _P(a), _P(b), _P(mask_a), _P(mask_b), n, d, ctx.chunks, _P(go), _P(gq), _P(ga),
                                              _P(gb), _lib.current_stream_ptr())
        _lib.check(rc, "ance_nll_backward")
        return gq, ga, gb, None, None


class _InBatchNLL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, ctxv, positive_idx):
        fn = "biencoder_nll_loss"
        _checked(q, fn + ": q", None)
        _checked(ctxv, fn + ": ctx", q.device)
        _checked(positive_idx, fn + ": positive_idx", q.device, torch.int64)
        if q.dim() != 2 or ctxv.dim() != 2 or q.shape[1] != ctxv.shape[1]:
            raise _lib.AnceLibraryError("%s: q [nq, d] and ctx [nc, d] expected, got %s and %s" % (fn, tuple(q.shape), tuple(ctxv.shape)))
        nq, d = q.shape
        nc = ctxv.shape[0]
        if tuple(positive_idx.shape) != (nq,):
            raise _lib.AnceLibraryError("%s: positive_idx has shape %s, expected (%d,)" % (fn, tuple(positive_idx.shape), nq))
        L = _lib.lib()
        need = L.ance_inbatch_nll_workspace_bytes(nq, nc, d)
        if need == 0:
            raise _lib.AnceLibraryError("%s: nq = %d, nc = %d, d = %d is outside 1 <= nq <= 1024, nq <= nc <= 2048, 128 <= d <= 1024, "
                                        "d %% 4 == 0" % (fn, nq, nc, d))
        ws = torch.empty(need, dtype=torch.uint8, device=q.device)
        mean = torch.empty((1,), dtype=torch.float32, device=q.device)
        counts = torch.empty((2,), dtype=torch.int64, device=q.device)
        with torch.cuda.device(q.device):
            rc = L.ance_inbatch_nll_forward(_P(q), _P(ctxv), _P(positive_idx), nq, nc, d, _P(mean), _P(counts), _P(ws), need,
                                            _lib.current_stream_ptr())
        _lib.check(rc, "ance_inbatch_nll_forward")
        ctx.save_for_backward(q, ctxv, positive_idx, ws)
        ctx.mark_non_differentiable(counts)
        return mean[0], counts

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, _grad_counts):
        q, ctxv, positive_idx, ws = ctx.saved_tensors
        nq, d = q.shape
        nc = ctxv.shape[0]
        go = _grad_output(grad_loss, q.device)
        gq, gc = torch.empty_like(q), torch.empty_like(ctxv)
        with torch.cuda.device(q.device):
            rc = _lib.lib().ance_inbatch_nll_backward(_P(q), _P(ctxv), _P(positive_idx), nq, nc, d, _P(go), _P(gq), _P(gc), _P(ws),
                                                      ws.numel(), _lib.current_stream_ptr())
        _lib.check(rc, "ance_inbatch_nll_backward")
        return gq, gc, None


def nll_loss(q, a, b, mask_a=None, mask_b=None, return_rows=False):
    """Mean over the n triplets of ``-log_softmax([q.a, q.b])[0]`` -- the tail of NLL.forward (model/models.py:77-81), of
    NLL_MultiChunk.forward (:103-134) and of BiEncoder.forward's triplet branch (:268-271) -- as a 0-dim tensor with a grad_fn.

    q [n, d]; a, b [n, d], or [n, chunks, d] with mask_a, mask_b [n, chunks] fp32: the first attention-mask entry of every chunk
    (an all-pad chunk is biased by -9999 before the max over chunks).  The gradient of a, b goes to the chunk that won the max, the
    lowest index among equal scores; every other chunk row is zero.  The value has the bits of ``AnceModel.forward``'s loss.
    return_rows: also the per-triplet logits [n, 2] and losses [n] (no gradient)."""
    loss, logits, rows = _TripletNLL.apply(q, a, b, mask_a, mask_b)
    return (loss, logits, rows) if return_rows else loss


def biencoder_nll_loss(q, ctx, positive_idx, return_invalid=False):
    """In-batch negatives (drivers/run_ann_dpr.py:356-365): ``scores = q ctx^T``, the mean of ``-log_softmax(scores)[i,
    positive_idx[i]]`` as a 0-dim tensor with a grad_fn, and the number of rows whose largest score (the lowest column among equal
    ones) is the positive, a 0-dim int64 device tensor.

    q [nq, d], ctx [nc, d] fp32, positive_idx [nq] int64 on the same device; 1 <= nq <= 1024, nq <= nc <= 2048, 128 <= d <= 1024,
    d % 4 == 0.  Gradients come back for all of q and ctx; rows that were concatenated from detached tensors (the other ranks' rows
    under DDP) are dropped by ``torch.cat``'s own backward.  A positive_idx outside [0, nc) reads and writes nothing out of bounds:
    the loss is NaN, so are that row's gradient contributions, the row never counts as correct; return_invalid adds the count of
    such rows (0-dim int64) to the result."""
    loss, counts = _InBatchNLL.apply(q, ctx, positive_idx)
    return (loss, counts[0], counts[1]) if return_invalid else (loss, counts[0])
