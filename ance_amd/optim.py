"""Fused LAMB for the ANCE trainers: a drop-in replacement of the reference's ``utils/lamb.py`` ``Lamb``, the optimizer
drivers/run_ann.py:80-84 and drivers/run_warmup.py:76-78 build when ``--optimizer lamb`` is passed (both launch recipes pass it).

The reference steps tensor by tensor in Python (about 19 small launches and up to three host synchronisations per tensor).
Here one call of ``ance_lamb_step`` (csrc/lamb.hip) updates every tensor of every group in three launches, with no host
synchronisation.  Same constructor, same errors, same state entries (``step`` an int, ``exp_avg``, ``exp_avg_sq``, and
``weight_norm``, ``adam_norm``, ``trust_ratio`` as 0-dim device tensors), so ``log_lamb_rs``, ``optimizer.state_dict()`` /
``torch.save`` and ``load_state_dict`` of the reference's ``optimizer.pt`` work unchanged, in both directions.

``max_grad_norm`` fuses the ``torch.nn.utils.clip_grad_norm_`` call every trainer of the reference makes in front of
``optimizer.step()`` (drivers/run_ann.py:283-289, run_ann_dpr.py:235-237) into the step (``ance_lamb_step_clipped``: five launches,
44 B per element, against 52 B and a dozen launches for the two calls).

Under ``torch.amp.GradScaler`` (the reference's ``--fp16`` recipe, drivers/run_ann.py:107-114,270-289, in its torch form) the step
speaks the scaler's contract for fused optimizers: ``_step_supports_amp_scaling`` is set, so ``scaler.step(optimizer)`` hands the
scale and the overflow flag over as device tensors and calls ``step()`` unconditionally; ``ance_lamb_step_amp`` unscales in
registers and skips on the device -- no host wait, no launch more, and the fused clip sees the unscaled gradients.

No CPU fallback: every parameter, gradient and state tensor must be a contiguous fp32 tensor on one HIP device.
"""
import ctypes

import numpy as np
import torch
from torch.optim import Optimizer

from . import _lib

# ctypes layout of AnceLambTensor (include/ance_amd.h), filled from a list of tuples in one call
_TENSOR_DTYPE = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("numel", "<i8"), ("group", "<i4"),
                          ("reserved", "<i4")])
_GROUP_DTYPE = np.dtype([("lr", "<f8"), ("beta1", "<f8"), ("beta2", "<f8"), ("eps", "<f8"), ("weight_decay", "<f8")])
assert _TENSOR_DTYPE.itemsize == ctypes.sizeof(_lib.AnceLambTensor)
assert _GROUP_DTYPE.itemsize == ctypes.sizeof(_lib.AnceLambGroup)


class Lamb(Optimizer):
    r"""LAMB (You et al., "Large Batch Optimization for Deep Learning: Training BERT in 76 minutes"), the reference's form:
    no bias correction, ``wn = min(|p|, 10)``, trust ratio 1 where ``wn`` or the Adam step's norm is 0, and ``adam=True``
    for a trust ratio of 1 always (the norms and the LAMB trust ratio are still recorded).

    Arguments as the reference's: params, lr (1e-3), betas ((0.9, 0.999)), eps (1e-6), weight_decay (0), adam (False).

    max_grad_norm (None, or a positive finite number): ``clip_grad_norm_(params, max_grad_norm)`` (2-norm,
    ``error_if_nonfinite=False``) over every parameter of every group that has a gradient, inside the step:
    ``coef = min(max_grad_norm / (total_norm + 1e-6), 1)`` in fp32 and every gradient element enters the moment updates as the fp32
    product ``g * coef``.  ``last_grad_norm`` is the total norm before clipping (what ``clip_grad_norm_`` returns) as a 0-dim device
    tensor, None before the first step.  The one visible difference from calling ``clip_grad_norm_``: ``p.grad`` is NOT rescaled in
    memory (the trainers zero the gradients right after the step).  A non-finite total norm makes ``coef`` NaN and poisons every
    stepped tensor, as torch's function does.  max_grad_norm is an attribute of the optimizer, not part of ``param_groups`` or
    ``state_dict()``: the reference's ``optimizer.pt`` stays byte-compatible.

    Loss scaling: ``torch.amp.GradScaler.step(optimizer)`` sets ``optimizer.grad_scale`` and ``optimizer.found_inf`` (one-element
    fp32 device tensors; either may be None) around its unconditional call of ``step()``.  With a ``grad_scale`` every gradient
    element enters the step as the fp32 product ``g * inv``, ``inv = float32(1 / float64(grad_scale))`` (what ``scaler.unscale_``
    multiplies by), formed in registers -- ``p.grad`` keeps its scaled bits -- and the clipping norm and ``last_grad_norm`` are
    those of the unscaled gradients: no ``scaler.unscale_(optimizer)`` is needed in front of the fused clip (after one,
    ``grad_scale`` arrives as None and only ``found_inf`` is honoured).  With a ``found_inf`` that is not 0 (NaN included) the step
    changes no bit of any parameter or moment, ``weight_norm`` / ``adam_norm`` / ``trust_ratio`` keep the previous step's values
    ((0, 0, 1) when there is none, or when the set of stepped parameters changed) and ``skipped_steps`` -- a 0-dim int64 device
    tensor, None until the first step under a scaler, not part of ``state_dict()`` -- grows by one; ``last_grad_norm`` is still
    written and may be inf or NaN.  ``state['step']`` cannot be un-incremented without a host wait: it counts calls, skipped
    ones included (no arithmetic reads it: the reference's LAMB has no bias correction).  A scale of 0 or a non-finite scale
    poisons the step.
    """
    _step_supports_amp_scaling = True  # torch.amp.GradScaler.step: attach grad_scale / found_inf and call step() unconditionally

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0, adam=False, max_grad_norm=None):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        if max_grad_norm is not None:
            try:
                ok = 0.0 < float(max_grad_norm) < float("inf")
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError("Invalid max_grad_norm: {} (None or a positive finite number)".format(max_grad_norm))
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.adam = adam
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = None
        self.skipped_steps = None
        super(Lamb, self).__init__(params, defaults)
        self._workspace = {}
        self._prev_out = None  # (out of the last step, the ids of the parameters its rows belong to)

    def _amp_scalar(self, name, device):
        """optimizer.grad_scale / optimizer.found_inf as GradScaler attaches them: None, or a one-element fp32 tensor on the step's
        device."""
        t = getattr(self, name, None)
        if t is None:
            return None
        what = "Lamb: optimizer.%s" % name
        _lib.require_cuda_tensor(t, torch.float32, what)
        if t.numel() != 1:
            raise _lib.AnceLibraryError("%s must have one element, got shape %s" % (what, tuple(t.shape)))
        if t.device != device:
            raise _lib.AnceLibraryError("%s is on %s, the parameters of this step on %s (mixed devices)" % (what, t.device, device))
        return t

    def _checked(self, t, what, device):
        _lib.require_cuda_tensor(t, torch.float32, what)
        if t.device != device:
            raise _lib.AnceLibraryError("%s is on %s, the other tensors of this step on %s (mixed devices)" % (what, t.device, device))
        return t

    def step(self, closure=None):
        """One LAMB step of every parameter that has a gradient.  Asynchronous: enqueued on the current stream, no host wait --
        also under a GradScaler (``grad_scale`` / ``found_inf``, see the class): a skipped step is skipped on the device."""
        loss = None
        if closure is not None:
            loss = closure()

        rows, groups, updated, stepped, device = [], [], [], [], None
        for gi, group in enumerate(self.param_groups):
            beta1, beta2 = group['betas']
            groups.append((float(group['lr']), float(beta1), float(beta2), float(group['eps']), float(group['weight_decay'])))
            for pi, p in enumerate(group['params']):
                if p.grad is None:
                    continue
                grad = p.grad
                if grad.is_sparse:
                    raise RuntimeError('Lamb does not support sparse gradients, consider SparseAdam instad.')
                name = "Lamb: param_groups[%d]['params'][%d]" % (gi, pi)
                if device is None:
                    _lib.require_cuda_tensor(p, torch.float32, name)
                    device = p.device
                self._checked(p, name, device)
                self._checked(grad, name + ".grad", device)
                if grad.shape != p.shape:
                    raise _lib.AnceLibraryError("%s.grad has shape %s, the parameter %s" % (name, tuple(grad.shape), tuple(p.shape)))
                state = self.state[p]
                if len(state) == 0:
                    state['step'] = 0
                    state['exp_avg'] = torch.zeros_like(p.data)
                    state['exp_avg_sq'] = torch.zeros_like(p.data)
                m, v = state['exp_avg'], state['exp_avg_sq']
                self._checked(m, name + " state['exp_avg']", device)
                self._checked(v, name + " state['exp_avg_sq']", device)
                if m.shape != p.shape or v.shape != p.shape:
                    raise _lib.AnceLibraryError("%s: state shapes %s, %s differ from the parameter's %s"
                                                % (name, tuple(m.shape), tuple(v.shape), tuple(p.shape)))
                rows.append((p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), gi, 0))
                updated.append(state)
                stepped.append(id(p))
        if not rows:
            return loss
        grad_scale, found_inf = self._amp_scalar("grad_scale", device), self._amp_scalar("found_inf", device)
        amp = grad_scale is not None or found_inf is not None

        L = _lib.lib()
        tensors = np.array(rows, dtype=_TENSOR_DTYPE)
        gtab = np.array(groups, dtype=_GROUP_DTYPE)
        total = int(tensors["numel"].sum())
        clip = self.max_grad_norm is not None
        size_fn = L.ance_lamb_amp_workspace_bytes if amp else L.ance_lamb_clipped_workspace_bytes if clip else L.ance_lamb_workspace_bytes
        need = size_fn(len(rows), len(groups), total)
        if need == 0:
            raise _lib.AnceLibraryError("Lamb: %d tensors of %d elements exceed ance_lamb_step's limits" % (len(rows), total))
        with torch.cuda.device(device):
            ws = self._workspace.get(device)
            if ws is None or ws.numel() < need:
                ws = torch.empty(need, dtype=torch.uint8, device=device)
                self._workspace[device] = ws
            out = torch.empty((len(rows), 3), dtype=torch.float32, device=device)
            stream = torch.cuda.current_stream(device).cuda_stream
            tab = (tensors.ctypes.data_as(ctypes.POINTER(_lib.AnceLambTensor)), len(rows),
                   gtab.ctypes.data_as(ctypes.POINTER(_lib.AnceLambGroup)), len(groups), 1 if self.adam else 0)
            tail = (ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ws.numel(), ctypes.c_void_p(stream))
            if amp:
                if self.skipped_steps is None or self.skipped_steps.device != device:
                    self.skipped_steps = torch.zeros((), dtype=torch.int64, device=device)
                prev = self._prev_out[0] if self._prev_out is not None and self._prev_out[1] == stepped else None
                norm = torch.empty((1,), dtype=torch.float32, device=device) if clip else None

                def ptr(t):
                    return None if t is None else ctypes.c_void_p(t.data_ptr())

                _lib.check(L.ance_lamb_step_amp(*tab, self.max_grad_norm if clip else 0.0, ptr(grad_scale), ptr(found_inf), ptr(prev),
                                                ptr(norm), ptr(self.skipped_steps), *tail), "ance_lamb_step_amp")
                if clip:
                    self.last_grad_norm = norm[0]
            elif clip:
                norm = torch.empty((1,), dtype=torch.float32, device=device)
                _lib.check(L.ance_lamb_step_clipped(*tab, self.max_grad_norm, ctypes.c_void_p(norm.data_ptr()), *tail),
                           "ance_lamb_step_clipped")
                self.last_grad_norm = norm[0]
            else:
                _lib.check(L.ance_lamb_step(*tab, *tail), "ance_lamb_step")
        self._prev_out = (out, stepped)
        vals = out.view(-1).unbind(0)
        for k, state in enumerate(updated):
            state['step'] += 1
            state['weight_norm'] = vals[3 * k]
            state['adam_norm'] = vals[3 * k + 1]
            state['trust_ratio'] = vals[3 * k + 2]
        return loss
