"""Fused optimizers for the ANCE trainers.  ``Lamb`` first; ``AdamW`` (transformers 2.3.0's, the DPR trainer's default) below it.

Fused LAMB: a drop-in replacement of the reference's ``utils/lamb.py`` ``Lamb``, the optimizer
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

``LossScaler`` (at the end) is the scaler with its whole state on the device: the fused step derives the overflow flag from the
gradient total it forms anyway (``ance_lamb_step_scaled`` / ``ance_adamw_step_scaled``) and ``update()`` is one launch
(``ance_loss_scale_update``), so ``scale`` / ``step`` / ``update`` can be captured in a graph with the rest of the step.

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
# AnceAdamwTensor
_ADAMW_TENSOR_DTYPE = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("step", "<u8"), ("numel", "<i8"),
                                ("group", "<i4"), ("reserved", "<i4")])
assert _ADAMW_TENSOR_DTYPE.itemsize == ctypes.sizeof(_lib.AnceAdamwTensor)


def _valid_max_grad_norm(max_grad_norm):
    if max_grad_norm is None:
        return None
    try:
        ok = 0.0 < float(max_grad_norm) < float("inf")
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("Invalid max_grad_norm: {} (None or a positive finite number)".format(max_grad_norm))
    return float(max_grad_norm)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class _Call(object):
    """What ``_FusedOptimizer.step`` hands to a subclass's ``_launch``: the library, the resident plan (``plan``: its sizes are the
    leading arguments of every planned entry point, ``tab``), the workspace and the stream, the scaler's tensors and what is stepped
    (``todo``: [(parameter, gradient, group index, state)]; ``group0``: the group of the first of them).  ``scaled``: the step runs
    under a ``LossScaler`` -- ``grad_scale`` and ``found_inf`` are its tensors and the step writes the flag itself."""
    __slots__ = ("L", "tab", "n", "device", "ws", "stream", "clip", "amp", "grad_scale", "found_inf", "todo", "group0", "plan", "scaled")


class _Plan(object):
    """The resident plan of a step: ``key`` (everything the device tables hold), ``ws`` (the device workspace the plan owns, the
    tables at its head), ``pinned`` (the host buffer they were uploaded from: never refilled while the plan lives, so a copy that
    a graph captured re-reads identical bytes) and the tables' sizes.  ``captured``: built or used while a graph was capturing."""
    __slots__ = ("key", "ws", "pinned", "n", "n_groups", "n_chunks", "captured", "lr_tensors")


class _FusedOptimizer(Optimizer):
    """What ``Lamb`` and ``AdamW`` share: the walk over ``param_groups`` with its checks, the host tables, the workspace cache, the
    scaler's contract.  A subclass names its table row (``_TENSOR_DTYPE``, ``_TENSOR_CTYPE``, ``_rows``), its state (``_init_state``,
    ``_check_state``), its workspace size and its library call (``_launch``)."""
    _step_supports_amp_scaling = True  # torch.amp.GradScaler.step: attach grad_scale / found_inf and call step() unconditionally
    _STATE_TENSORS = (('exp_avg', " state['exp_avg']"), ('exp_avg_sq', " state['exp_avg_sq']"))   # checked in this order
    _PINNED_MIN = 65536

    # ---- the resident plan.  The device tables of a step (tensor rows, chunk map, group rows) are built once and live in memory
    # the plan owns; a step whose key -- every pointer and numel, every group hyper-parameter but a device lr, the clip, amp and
    # subclass flags -- equals the plan's builds no table, copies nothing and enqueues only its kernels.  Any difference rebuilds.
    def _plan_init(self):
        self._plan = None
        self._kept_plans = []    # plans a captured graph may still refer to: alive as long as the optimizer is
        self._spare_pinned = None  # allocated outside capture, so that a rebuild during capture allocates no pinned memory

    def invalidate_plan(self):
        """Drops the resident plan: the next ``step()`` rebuilds it.  Needed only when something the plan cannot see changed.  A
        graph captured earlier keeps replaying the plan it captured (which stays alive as long as this optimizer does) --
        re-capturing after ``invalidate_plan()`` is the caller's job."""
        plan = self._plan
        if plan is not None and plan.captured:
            self._kept_plans.append(plan)
        self._plan = None

    def _take_pinned(self, nbytes, capturing):
        spare = self._spare_pinned
        if spare is not None and spare.numel() >= nbytes:
            buf, self._spare_pinned = spare, None
        else:
            size = self._PINNED_MIN
            while size < nbytes:
                size <<= 1
            buf = torch.empty(size, dtype=torch.uint8, pin_memory=True)
        if not capturing and self._spare_pinned is None:
            self._spare_pinned = torch.empty(buf.numel(), dtype=torch.uint8, pin_memory=True)
        return buf

    def _build_plan(self, key, rows, groups, lrs, c, capturing):
        L, n_groups = c.L, len(groups)
        tensors = np.array(rows, dtype=self._TENSOR_DTYPE)
        gtab = np.array(groups, dtype=_GROUP_DTYPE)
        total = int(tensors["numel"].sum())
        need = self._workspace_bytes(c, n_groups, total)
        table_bytes = getattr(L, self._PLAN + "_plan_table_bytes")(c.n, n_groups, total)
        if need == 0 or table_bytes == 0:
            raise _lib.AnceLibraryError("%s: %d tensors of %d elements exceed %s's limits" % (self._name, c.n, total, self._ENTRY))
        self.invalidate_plan()
        plan = _Plan()
        plan.key, plan.n, plan.n_groups, plan.captured = key, c.n, n_groups, capturing
        plan.lr_tensors = [lr for lr in lrs if lr is not None]   # the plan holds their pointers
        plan.pinned = self._take_pinned(table_bytes, capturing)
        plan.ws = torch.empty(need, dtype=torch.uint8, device=c.device)   # torch's allocator: a graph's own pool while capturing
        d_lrs = None
        if plan.lr_tensors:
            d_lrs = (ctypes.c_void_p * n_groups)(*[None if lr is None else lr.data_ptr() for lr in lrs])
        n_chunks, filled = ctypes.c_int64(0), ctypes.c_size_t(0)
        _lib.check(getattr(L, self._PLAN + "_plan_build")(tensors.ctypes.data_as(ctypes.POINTER(self._TENSOR_CTYPE)), c.n,
                                                          gtab.ctypes.data_as(ctypes.POINTER(_lib.AnceLambGroup)), d_lrs, n_groups,
                                                          ctypes.c_void_p(plan.pinned.data_ptr()), plan.pinned.numel(),
                                                          ctypes.byref(n_chunks), ctypes.byref(filled)), self._PLAN + "_plan_build")
        plan.n_chunks = n_chunks.value
        plan.ws[:filled.value].copy_(plan.pinned[:filled.value], non_blocking=True)   # the one upload of the plan's life
        self._plan = plan
        self._workspace[c.device] = plan.ws
        return plan

    def _group_lr(self, gi, group):
        """(the host lr, None) or (0.0, the device lr): a 0-dim float64 CUDA tensor, as torch's capturable optimizers accept."""
        lr = group['lr']
        if not isinstance(lr, torch.Tensor):
            return float(lr), None
        if not lr.is_cuda or lr.dtype != torch.float64 or lr.numel() != 1:
            raise _lib.AnceLibraryError("%s: param_groups[%d]['lr'] as a tensor must be a 0-dim float64 CUDA tensor, got %s %s on %s"
                                        % (self._name, gi, tuple(lr.shape), lr.dtype, lr.device))
        return 0.0, lr

    def _amp_scalar(self, name, device):
        """optimizer.grad_scale / optimizer.found_inf as GradScaler attaches them: None, or a one-element fp32 tensor on the step's
        device."""
        t = getattr(self, name, None)
        if t is None:
            return None
        what = "%s: optimizer.%s" % (self._name, name)
        _lib.require_cuda_tensor(t, torch.float32, what)
        if t.numel() != 1:
            raise _lib.AnceLibraryError("%s must have one element, got shape %s" % (what, tuple(t.shape)))
        if t.device != device:
            raise _lib.AnceLibraryError("%s is on %s, the parameters of this step on %s (mixed devices)" % (what, t.device, device))
        return t

    def _checked(self, t, what, device):
        if isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == device:
            return t   # the common case in one test: several tensors per parameter pass here at every step
        _lib.require_cuda_tensor(t, torch.float32, what)
        if t.device != device:
            raise _lib.AnceLibraryError("%s is on %s, the other tensors of this step on %s (mixed devices)" % (what, t.device, device))
        return t

    def _check_group(self, gi, group, first_group):
        """A subclass's check of a group that has a parameter to step; first_group: the first such group."""

    def _check_state(self, state, name, p, device):
        for key, suffix in self._STATE_TENSORS:
            self._checked(state[key], name + suffix, device)
        m, v = state['exp_avg'], state['exp_avg_sq']
        if m.shape != p.shape or v.shape != p.shape:
            raise _lib.AnceLibraryError("%s: state shapes %s, %s differ from the parameter's %s"
                                        % (name, tuple(m.shape), tuple(v.shape), tuple(p.shape)))

    def _walk(self):
        """([(parameter, gradient, group index, its state or None)] of the parameters that have a gradient, the group table, the
        groups' device learning rates (None where the lr is a host number), their device).  Checks everything and changes nothing:
        a refused step leaves no entry in ``self.state`` behind."""
        todo, groups, lrs, device, first_group = [], [], [], None, None
        checked, check_state, state_of = self._checked, self._check_state, self.state.get   # .get: no entry is created
        for gi, group in enumerate(self.param_groups):
            beta1, beta2 = group['betas']
            lr, d_lr = self._group_lr(gi, group)
            lrs.append(d_lr)
            groups.append((lr, float(beta1), float(beta2), float(group['eps']), float(group['weight_decay'])))
            group_checked = False
            for pi, p in enumerate(group['params']):
                if p.grad is None:
                    continue
                grad = p.grad
                if grad.is_sparse:
                    raise RuntimeError(self._SPARSE)
                name = "%s: param_groups[%d]['params'][%d]" % (self._name, gi, pi)
                if device is None:
                    _lib.require_cuda_tensor(p, torch.float32, name)
                    device, first_group = p.device, group
                checked(p, name, device)
                checked(grad, name + ".grad", device)
                if grad.shape != p.shape:
                    raise _lib.AnceLibraryError("%s.grad has shape %s, the parameter %s" % (name, tuple(grad.shape), tuple(p.shape)))
                if not group_checked:
                    self._check_group(gi, group, first_group)
                    group_checked = True
                state = state_of(p)
                if state:
                    check_state(state, name, p, device)
                todo.append((p, grad, gi, state))
        for gi, lr in enumerate(lrs):
            if lr is not None and device is not None and lr.device != device:
                raise _lib.AnceLibraryError("%s: param_groups[%d]['lr'] is on %s, the parameters of this step on %s (mixed devices)"
                                            % (self._name, gi, lr.device, device))
        return todo, groups, lrs, device

    def step(self, closure=None):
        """One step of every parameter that has a gradient.  Asynchronous: enqueued on the current stream, no host wait -- also
        under a GradScaler (``grad_scale`` / ``found_inf``, see the class): a skipped step is skipped on the device."""
        loss = None
        if closure is not None:
            loss = closure()

        todo, groups, lrs, device = self._walk()
        scaler = getattr(self, "_loss_scaler", None)   # set by LossScaler.step around this call only
        if not todo:
            if scaler is not None:
                raise RuntimeError("%s: LossScaler.step found no parameter with a gradient: no overflow check was made" % self._name)
            return loss
        c = _Call()
        c.group0 = self.param_groups[todo[0][2]]
        c.scaled = scaler is not None
        if c.scaled:
            c.grad_scale, c.found_inf = scaler._tensors_on(device, self._name)
        else:
            c.grad_scale, c.found_inf = self._amp_scalar("grad_scale", device), self._amp_scalar("found_inf", device)
        c.amp = c.grad_scale is not None or c.found_inf is not None
        for k, (p, grad, gi, state) in enumerate(todo):   # everything is checked: only now is state created
            if not state:
                state = self.state[p]
                self._init_state(state, p)
                todo[k] = (p, grad, gi, state)
        c.todo = todo
        rows = self._rows(todo)

        c.L = _lib.lib()
        c.n, c.device, c.clip = len(rows), device, self.max_grad_norm is not None
        key = (rows, groups, [None if lr is None else lr.data_ptr() for lr in lrs], c.clip, c.amp, self._plan_flags(c), device, c.scaled)
        capturing = torch.cuda.is_current_stream_capturing()
        with torch.cuda.device(device):
            plan = self._plan
            if plan is None or plan.key != key:
                plan = self._build_plan(key, rows, groups, lrs, c, capturing)
            elif capturing:
                plan.captured = True
            c.plan, c.ws = plan, plan.ws
            if c.amp and (self.skipped_steps is None or self.skipped_steps.device != device):
                self.skipped_steps = torch.zeros((), dtype=torch.int64, device=device)
            c.stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            c.tab = (plan.n, plan.n_groups, plan.n_chunks)
            self._launch(c)
        return loss


class Lamb(_FusedOptimizer):
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
    _name = "Lamb"  # in front of every AnceLibraryError
    _ENTRY, _PLAN = "ance_lamb_step", "ance_lamb"
    _SPARSE = 'Lamb does not support sparse gradients, consider SparseAdam instad.'
    _TENSOR_DTYPE, _TENSOR_CTYPE = _TENSOR_DTYPE, _lib.AnceLambTensor

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0, adam=False, max_grad_norm=None):
        if not isinstance(lr, torch.Tensor) and not 0.0 <= lr:   # a device lr is not read back: that would be a host wait
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        max_grad_norm = _valid_max_grad_norm(max_grad_norm)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.adam = adam
        self.max_grad_norm = max_grad_norm
        self.last_grad_norm = None
        self.skipped_steps = None
        super(Lamb, self).__init__(params, defaults)
        self._workspace = {}
        self._plan_init()
        self._prev_out = None  # (out of the last step, the ids of the parameters its rows belong to)
        self._scaled_out = None  # the same under a LossScaler: one persistent buffer

    def _plan_flags(self, c):
        return bool(self.adam)

    def _init_state(self, state, p):
        state['step'] = 0
        state['exp_avg'] = torch.zeros_like(p.data)
        state['exp_avg_sq'] = torch.zeros_like(p.data)

    def _rows(self, todo):
        return [(p.data_ptr(), grad.data_ptr(), state['exp_avg'].data_ptr(), state['exp_avg_sq'].data_ptr(), p.numel(), gi, 0)
                for p, grad, gi, state in todo]

    def _workspace_bytes(self, c, n_groups, total):
        L = c.L
        size_fn = L.ance_lamb_amp_workspace_bytes if c.amp else L.ance_lamb_clipped_workspace_bytes if c.clip else L.ance_lamb_workspace_bytes
        return size_fn(c.n, n_groups, total)

    def _launch(self, c):
        L, device, clip = c.L, c.device, c.clip
        stepped = [id(t[0]) for t in c.todo]
        norm = torch.empty((1,), dtype=torch.float32, device=device) if clip else None
        if c.scaled:
            # one buffer as long as the same parameters are stepped, handed in as its own d_prev_out: a skipped step, eager or
            # replayed from a graph, keeps the rows of the step before it ((0, 0, 1) before the first).  It outlives a rebuild of
            # the plan (new gradient tensors at a capture), so the buffer a graph holds is the one the warm-up steps made
            kept = self._scaled_out
            if kept is None or kept[1] != stepped or kept[0].device != device:
                out = torch.zeros((c.n, 3), dtype=torch.float32, device=device)
                out[:, 2] = 1.0
                self._scaled_out = (out, stepped)
            else:
                out = kept[0]
            entry, prev = "ance_lamb_step_scaled", out
        else:
            out = torch.empty((c.n, 3), dtype=torch.float32, device=device)
            prev = self._prev_out[0] if c.amp and self._prev_out is not None and self._prev_out[1] == stepped else None
            entry = "ance_lamb_step_planned"
        _lib.check(getattr(L, entry)(*c.tab, 1 if self.adam else 0, self.max_grad_norm if clip else 0.0, _ptr(c.grad_scale),
                                     _ptr(c.found_inf), _ptr(prev), _ptr(norm), _ptr(self.skipped_steps if c.amp else None),
                                     ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(c.ws.data_ptr()), c.ws.numel(), c.stream), entry)
        if clip:
            self.last_grad_norm = norm[0]
        self._prev_out = (out, stepped)
        vals = out.view(-1).unbind(0)
        for k, (_, _, _, state) in enumerate(c.todo):
            state['step'] += 1
            state['weight_norm'] = vals[3 * k]
            state['adam_norm'] = vals[3 * k + 1]
            state['trust_ratio'] = vals[3 * k + 2]


class AdamW(_FusedOptimizer):
    r"""AdamW as transformers 2.3.0 has it (optimization.py, ``AdamW``) -- the optimizer drivers/run_ann_dpr.py:501-504 makes the DPR
    trainer's default through utils/dpr_utils.py:80-92, and run_ann.py:85-89 / run_warmup.py:79-81 build for ``--optimizer adamW``.
    transformers 5 no longer has the class, and ``torch.optim.AdamW`` is another arithmetic: it decays before the update and puts
    ``eps`` inside the bias correction.  Here, per tensor::

        m <- beta1 m + (1 - beta1) g ;  v <- beta2 v + (1 - beta2) g g ;  t = step + 1
        ss = lr sqrt(1 - beta2^t) / (1 - beta1^t)          (lr when correct_bias is False)
        p <- p - ss m / (sqrt(v) + eps) ;  then p <- p - lr weight_decay p on the UPDATED p when weight_decay > 0

    One call of ``ance_adamw_step`` (csrc/adamw.hip) steps every tensor of every group: two launches (28 B per element), three with
    ``max_grad_norm`` (32 B), no host synchronisation.

    Arguments as 2.3.0's: params, lr (1e-3), betas ((0.9, 0.999)), eps (1e-6), weight_decay (0.0), correct_bias (True), and
    ``max_grad_norm`` as ``Lamb``'s: ``clip_grad_norm_`` fused in front (``last_grad_norm``; ``p.grad`` is not rescaled in memory).
    ``correct_bias`` is a group default as in 2.3.0, but one step has one value: groups that disagree are refused.

    ``state['step']`` is a 0-dim fp32 DEVICE tensor (what torch's fused Adam keeps; exact up to 2^24 steps), advanced by the kernel:
    the count enters the bias correction, so a step skipped for overflow must not advance it, and only the device knows.  A
    parameter without a gradient is skipped and gets no state, so under ``find_unused_parameters=True`` tensors carry different
    counts and each uses its own bias correction.  A parameter of no elements keeps ``step`` 0.

    Loss scaling exactly as ``Lamb``'s (``_step_supports_amp_scaling``; ``grad_scale`` / ``found_inf`` attached by
    ``torch.amp.GradScaler.step``): unscale in registers, the clipping norm over the unscaled gradients, and with a ``found_inf``
    that is not 0 (NaN included) no bit of any parameter, moment or ``step`` changes and ``skipped_steps`` grows by one.

    Resume: ``state_dict()`` returns ``step`` as a Python int (one device read per save, off the step path), the layout 2.3.0 writes
    and reads; ``load_state_dict`` takes that layout (int steps, CPU tensors) as well as tensors and moves ``step`` to the device as
    fp32.  ``max_grad_norm`` is an attribute, not part of ``param_groups`` or ``state_dict()``.

    No CPU fallback: every parameter, gradient and state tensor must be a contiguous fp32 tensor on one HIP device.
    """
    _name = "AdamW"
    _ENTRY, _PLAN = "ance_adamw_step", "ance_adamw"
    _SPARSE = 'Adam does not support sparse gradients, please consider SparseAdam instead'
    _TENSOR_DTYPE, _TENSOR_CTYPE = _ADAMW_TENSOR_DTYPE, _lib.AnceAdamwTensor
    _STATE_TENSORS = _FusedOptimizer._STATE_TENSORS + (('step', " state['step']"),)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, correct_bias=True, max_grad_norm=None):
        if not isinstance(lr, torch.Tensor) and lr < 0.0:   # a device lr is not read back: that would be a host wait
            raise ValueError("Invalid learning rate: {} - should be >= 0.0".format(lr))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[1]))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {} - should be >= 0.0".format(eps))
        self.max_grad_norm = _valid_max_grad_norm(max_grad_norm)
        self.last_grad_norm = None
        self.skipped_steps = None
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, correct_bias=correct_bias)
        super(AdamW, self).__init__(params, defaults)
        self._workspace = {}
        self._plan_init()

    def _plan_flags(self, c):
        return bool(c.group0['correct_bias'])

    def state_dict(self):
        """The reference's layout: ``step`` a Python int.  One device read for all of them."""
        sd = super(AdamW, self).state_dict()
        keys = [k for k, s in sd["state"].items() if isinstance(s.get("step"), torch.Tensor)]
        if keys:
            steps = torch.stack([sd["state"][k]["step"].detach().reshape(()).float() for k in keys]).cpu().tolist()
            sd["state"] = dict(sd["state"])
            for k, n in zip(keys, steps):
                sd["state"][k] = dict(sd["state"][k], step=int(n))   # a copy: the live state keeps its device tensor
        return sd

    def load_state_dict(self, state_dict):
        """Accepts ``step`` as an int (the reference's and this class's files) or a tensor; it lives on the parameter's device."""
        super(AdamW, self).load_state_dict(state_dict)
        for group in self.param_groups:
            for p in group['params']:
                st = self.state.get(p)
                if st and 'step' in st:
                    n = st['step']
                    n = float(n.item()) if isinstance(n, torch.Tensor) else float(n)
                    st['step'] = torch.full((), n, dtype=torch.float32, device=p.device)

    def _check_group(self, gi, group, first_group):
        if bool(group['correct_bias']) != bool(first_group['correct_bias']):
            raise _lib.AnceLibraryError("AdamW: param_groups[%d]['correct_bias'] differs from an earlier group's: one step "
                                        "has one value" % gi)

    def _check_state(self, state, name, p, device):
        _FusedOptimizer._check_state(self, state, name, p, device)
        n = state['step']
        if n.numel() != 1:
            raise _lib.AnceLibraryError("%s: state['step'] must have one element, got shape %s" % (name, tuple(n.shape)))

    def _init_state(self, state, p):
        state['step'] = torch.zeros((), dtype=torch.float32, device=p.device)
        state['exp_avg'] = torch.zeros_like(p.data)
        state['exp_avg_sq'] = torch.zeros_like(p.data)

    def _rows(self, todo):
        return [(p.data_ptr(), grad.data_ptr(), state['exp_avg'].data_ptr(), state['exp_avg_sq'].data_ptr(), state['step'].data_ptr(),
                 p.numel(), gi, 0) for p, grad, gi, state in todo]

    def _workspace_bytes(self, c, n_groups, total):
        return c.L.ance_adamw_workspace_bytes(c.n, n_groups, total, 1 if c.clip or c.scaled else 0)

    def _launch(self, c):
        """A skipped step is skipped on the device, its step counts included."""
        norm = torch.empty((1,), dtype=torch.float32, device=c.device) if c.clip else None
        entry = "ance_adamw_step_scaled" if c.scaled else "ance_adamw_step_planned"
        _lib.check(getattr(c.L, entry)(*c.tab, 1 if c.group0['correct_bias'] else 0, self.max_grad_norm if c.clip else 0.0,
                                       _ptr(c.grad_scale), _ptr(c.found_inf), _ptr(norm),
                                       _ptr(self.skipped_steps if c.amp else None), ctypes.c_void_p(c.ws.data_ptr()),
                                       c.ws.numel(), c.stream), entry)
        if c.clip:
            self.last_grad_norm = norm[0]


class LinearWarmupSchedule(object):
    r"""``transformers.get_linear_schedule_with_warmup(optimizer, num_warmup_steps, num_training_steps)`` on the device: the schedule
    every trainer of the reference steps after ``optimizer.step()`` (drivers/run_ann.py:175,290, run_warmup.py:87,218,
    run_ann_dpr.py:110,240), with the step count and every group's learning rate in device memory, so that a captured training
    step carries its schedule and a replay applies the lr of the step it stands for.

    Construction turns every ``param_groups[i]['lr']`` into a 0-dim float64 device tensor (views of one array; ``Lamb`` and ``AdamW``
    read them at every step with no rebuild of their plan), keeps ``base_lrs`` and applies ``n = 0`` as ``LambdaLR`` does.
    ``step()`` is ONE launch (csrc/lr_schedule.hip), capturable and without a host wait: ``n += 1``, then
    ``lr_g = base_g * lambda(n)`` in fp64, ``lambda(n) = n / max(1, warm)`` below ``warm``, else
    ``max(0, (total - n) / max(1, total - warm))`` -- the values ``LambdaLR`` holds, bit for bit.  The count advances on every call,
    also after a step the scaler skipped, as the reference's ``scheduler.step()`` does.
    ``get_last_lr()``, ``state_dict()`` and ``load_state_dict()`` each take one device read: off the step path."""

    def __init__(self, optimizer, num_warmup_steps, num_training_steps, device=None):
        self.optimizer = optimizer
        self.num_warmup_steps, self.num_training_steps = int(num_warmup_steps), int(num_training_steps)
        groups = optimizer.param_groups
        if device is None:
            found = [p.device for g in groups for p in g['params']]
            if not found or not found[0].type == "cuda":
                raise _lib.AnceLibraryError("LinearWarmupSchedule: the optimizer's parameters must be on a HIP device")
            device = found[0]
        self.device = torch.device(device)
        base = []
        for g in groups:
            lr = g.get('initial_lr', g['lr'])
            base.append(float(lr))   # a tensor lr is read back here, once
            g.setdefault('initial_lr', base[-1])
        self.base_lrs = base
        self._base = torch.tensor(base, dtype=torch.float64, device=self.device)
        self._lrs = torch.zeros(len(base), dtype=torch.float64, device=self.device)
        self._n = torch.full((), -1, dtype=torch.int64, device=self.device)
        for k, g in enumerate(groups):
            g['lr'] = self._lrs[k]
        self.step()   # n = 0

    def step(self):
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ance_linear_warmup_step(ctypes.c_void_p(self._n.data_ptr()), ctypes.c_void_p(self._base.data_ptr()),
                                                          ctypes.c_void_p(self._lrs.data_ptr()), len(self.base_lrs), self.num_warmup_steps,
                                                          self.num_training_steps, _lib.current_stream_ptr()),
                       "ance_linear_warmup_step")

    def get_last_lr(self):
        """The groups' current learning rates as Python floats: one device read."""
        return self._lrs.tolist()

    def state_dict(self):
        """``LambdaLR``'s entries that matter: ``last_epoch``, ``base_lrs``, ``_last_lr``.  One device read."""
        vals = torch.cat([self._n.reshape(1).to(torch.float64), self._lrs]).tolist()
        return dict(last_epoch=int(vals[0]), base_lrs=list(self.base_lrs), _last_lr=vals[1:],
                    num_warmup_steps=self.num_warmup_steps, num_training_steps=self.num_training_steps)

    def load_state_dict(self, state_dict):
        """Takes this class's and ``LambdaLR``'s state dicts: the count and the base lrs; the learning rates follow from them."""
        base = [float(x) for x in state_dict.get("base_lrs", self.base_lrs)]
        if len(base) != len(self.base_lrs):
            raise ValueError("loaded state dict has %d base_lrs, the optimizer %d groups" % (len(base), len(self.base_lrs)))
        self.num_warmup_steps = int(state_dict.get("num_warmup_steps", self.num_warmup_steps))
        self.num_training_steps = int(state_dict.get("num_training_steps", self.num_training_steps))
        self.base_lrs = base
        self._base.copy_(torch.tensor(base, dtype=torch.float64))
        self._n.fill_(int(state_dict["last_epoch"]) - 1)
        self.step()



def _positive_finite(name, x):
    try:
        ok = 0.0 < float(x) < float("inf")
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("Invalid {}: {} (a positive finite number)".format(name, x))
    return float(x)


class LossScaler(object):
    r"""Dynamic loss scaling for ``Lamb`` / ``AdamW`` with the scaler's whole state on the device: ``torch.amp.GradScaler``'s recipe
    (``scale`` -> ``backward`` -> ``step`` -> ``update``) without its pass over the gradients and without its walk over the parameters,
    so that a captured training step carries its scaler::

        scaler = LossScaler(init_scale=65536.0, growth_interval=2000)
        scaler.scale(loss).backward()
        scaler.step(optimizer)     # the fused step unscales in registers, finds its own overflow and skips on the device
        scaler.update()            # one launch: torch._amp_update_scale_'s arithmetic, bit for bit

    ``step`` calls the optimizer through ``ance_lamb_step_scaled`` / ``ance_adamw_step_scaled``: the gradient-norm pass (which the
    fused clip makes anyway; it also runs without ``max_grad_norm``) totals the squares of the unscaled gradient elements ``g * inv``
    in fp64, and the step is skipped exactly when that total is not finite.  For a scale >= 1 that is ``GradScaler``'s rule (some
    gradient element is inf or NaN); for a scale below 1 it also catches a finite element whose unscaled product overflows.
    ``optimizer.skipped_steps``, ``last_grad_norm`` and LAMB's recorded norms behave as under a ``GradScaler``; a skipped LAMB step
    keeps the previous step's norms, also when replayed from a graph (one persistent buffer per plan).

    State: ``scale`` (fp32 [1]), ``growth_tracker`` (int32 [1]) and ``found_inf`` (fp32 [1]) are created at the first ``scale()`` on
    that tensor's device and kept for life -- a captured graph holds their addresses; everything later fills them in place.
    Nothing in ``scale``, ``step`` or ``update`` waits for the device, and all three can be captured (after a first eager use).
    ``get_scale()``, ``state_dict()`` and ``load_state_dict()`` read or fill the device tensors off the step path; the state dict has
    ``GradScaler``'s keys, so a checkpoint moves between the two classes.

    One optimizer per scaler; ``unscale_`` is refused (the fused clip already works on the unscaled gradients).  ``enabled=False``:
    every method passes through and ``step`` calls ``optimizer.step()``."""

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True):
        self._enabled = bool(enabled)
        self._init_scale = _positive_finite("init_scale", init_scale)
        self._growth_factor = _positive_finite("growth_factor", growth_factor)
        self._backoff_factor = _positive_finite("backoff_factor", backoff_factor)
        if int(growth_interval) != growth_interval or int(growth_interval) < 1:
            raise ValueError("Invalid growth_interval: {} (an integer >= 1)".format(growth_interval))
        self._growth_interval = int(growth_interval)
        self._init_growth_tracker = 0
        self.scale_tensor = self.growth_tracker = self.found_inf = None   # device tensors, from the first scale() on
        self._scale0 = None   # a 0-dim view of scale_tensor: what outputs are multiplied by

    def is_enabled(self):
        return self._enabled

    # ---- state
    def _create(self, device):
        if torch.cuda.is_current_stream_capturing():
            raise _lib.AnceLibraryError("LossScaler: the first scale() creates the scaler's device state and cannot be captured: "
                                        "run a step outside the capture first")
        self.scale_tensor = torch.full((1,), self._init_scale, dtype=torch.float32, device=device)
        self.growth_tracker = torch.full((1,), self._init_growth_tracker, dtype=torch.int32, device=device)
        self.found_inf = torch.zeros((1,), dtype=torch.float32, device=device)
        self._scale0 = self.scale_tensor[0]

    def _tensors_on(self, device, who):
        """(scale, found_inf) for a step of ``who`` on ``device``."""
        if self.scale_tensor is None:
            raise RuntimeError("LossScaler.step: no scale() came before it: there are no scaled gradients to step on")
        if self.scale_tensor.device != device:
            raise _lib.AnceLibraryError("%s: the LossScaler's state is on %s, the parameters of this step on %s (mixed devices)"
                                        % (who, self.scale_tensor.device, device))
        return self.scale_tensor, self.found_inf

    # ---- the step path: no host wait, capturable
    def scale(self, outputs):
        """``outputs * scale`` by the device scalar, for a tensor or an iterable of tensors, as ``GradScaler.scale``."""
        if not self._enabled:
            return outputs
        if isinstance(outputs, torch.Tensor):
            if not outputs.is_cuda:
                raise _lib.AnceLibraryError("LossScaler.scale: outputs must be on a HIP device, got %s" % outputs.device)
            if self.scale_tensor is None:
                self._create(outputs.device)
            elif self.scale_tensor.device != outputs.device:
                raise _lib.AnceLibraryError("LossScaler.scale: outputs are on %s, the scaler's state on %s (mixed devices)"
                                            % (outputs.device, self.scale_tensor.device))
            return outputs * self._scale0
        if isinstance(outputs, (list, tuple)) or hasattr(outputs, "__iter__"):
            mapped = [self.scale(o) for o in outputs]
            return type(outputs)(mapped) if isinstance(outputs, (list, tuple)) else mapped
        raise ValueError("outputs must be a Tensor or an iterable of Tensors")

    def step(self, optimizer, *args, **kwargs):
        """One step of ``optimizer`` -- a ``Lamb`` or ``AdamW`` of this module -- on the scaled gradients: unscaled in registers,
        skipped on the device when an unscaled gradient element is not finite.  Returns what ``optimizer.step`` returns."""
        if not self._enabled:
            return optimizer.step(*args, **kwargs)
        if not isinstance(optimizer, _FusedOptimizer):
            raise TypeError("LossScaler.step takes an ance_amd.optim.Lamb or ance_amd.optim.AdamW, got %s.%s: use "
                            "torch.amp.GradScaler for other optimizers"
                            % (type(optimizer).__module__, type(optimizer).__name__))
        if "closure" in kwargs or args:
            raise RuntimeError("Closure use is not currently supported if LossScaler is enabled.")
        if getattr(optimizer, "grad_scale", None) is not None or getattr(optimizer, "found_inf", None) is not None:
            raise RuntimeError("LossScaler.step: %s.grad_scale / found_inf are set: the optimizer is being driven by another scaler"
                               % optimizer._name)
        optimizer._loss_scaler = self
        try:
            return optimizer.step()
        finally:
            optimizer._loss_scaler = None

    def unscale_(self, optimizer):
        raise RuntimeError("LossScaler.unscale_ is not supported: the fused clip (max_grad_norm) of Lamb / AdamW already works on the "
                           "unscaled gradients, and the step unscales in registers")

    def update(self, new_scale=None):
        """After ``step``: back off on an overflow, grow after ``growth_interval`` clean steps -- one launch.  With ``new_scale`` (a
        float or a one-element tensor) the scale is filled in place instead, as ``GradScaler.update`` does."""
        if not self._enabled:
            return
        if self.scale_tensor is None:
            raise RuntimeError("LossScaler.update: no scale() came before it")
        if new_scale is not None:
            if isinstance(new_scale, torch.Tensor):
                if new_scale.numel() != 1 or new_scale.requires_grad:
                    raise ValueError("new_scale must be a one-element tensor with requires_grad=False")
                if not new_scale.is_cuda and torch.cuda.is_current_stream_capturing():
                    raise _lib.AnceLibraryError("LossScaler.update: new_scale is a host tensor and a copy from the host cannot be "
                                                "captured: pass a device tensor or a float")
                self.scale_tensor.copy_(new_scale.detach().reshape(1))
            else:
                self.scale_tensor.fill_(_positive_finite("new_scale", new_scale))
            return
        with torch.cuda.device(self.scale_tensor.device):
            _lib.check(_lib.lib().ance_loss_scale_update(ctypes.c_void_p(self.scale_tensor.data_ptr()),
                                                         ctypes.c_void_p(self.growth_tracker.data_ptr()),
                                                         ctypes.c_void_p(self.found_inf.data_ptr()), self._growth_factor,
                                                         self._backoff_factor, self._growth_interval, _lib.current_stream_ptr()),
                       "ance_loss_scale_update")

    # ---- read-outs and checkpoints: off the step path
    def get_scale(self):
        """The scale as a Python float: one synchronising read (``init_scale`` before the first ``scale()``)."""
        if not self._enabled:
            return 1.0
        return self._init_scale if self.scale_tensor is None else float(self.scale_tensor.item())

    def get_growth_factor(self):
        return self._growth_factor

    def get_backoff_factor(self):
        return self._backoff_factor

    def get_growth_interval(self):
        return self._growth_interval

    def _get_growth_tracker(self):
        if not self._enabled:
            return 0
        return self._init_growth_tracker if self.growth_tracker is None else int(self.growth_tracker.item())

    def state_dict(self):
        """``torch.amp.GradScaler.state_dict()``'s keys and meanings; ``{}`` when disabled."""
        if not self._enabled:
            return {}
        return {"scale": self.get_scale(), "growth_factor": self._growth_factor, "backoff_factor": self._backoff_factor,
                "growth_interval": self._growth_interval, "_growth_tracker": self._get_growth_tracker()}

    def load_state_dict(self, state_dict):
        """Takes this class's and ``torch.amp.GradScaler``'s state dicts; device tensors that exist are filled in place."""
        if not self._enabled:
            return
        if len(state_dict) == 0:
            raise RuntimeError("The source state dict is empty, possibly because it was saved from a disabled instance of GradScaler.")
        self._init_scale = _positive_finite("scale", state_dict["scale"])
        self._growth_factor = _positive_finite("growth_factor", state_dict["growth_factor"])
        self._backoff_factor = _positive_finite("backoff_factor", state_dict["backoff_factor"])
        self._growth_interval = int(state_dict["growth_interval"])
        self._init_growth_tracker = int(state_dict["_growth_tracker"])
        if self.scale_tensor is not None:
            self.scale_tensor.fill_(self._init_scale)
            self.growth_tracker.fill_(self._init_growth_tracker)
