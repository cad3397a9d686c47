"""Loss and optimizer of the reference's training step (/root/reference/PathNet_run.py:295-297, :346-352) as single
launches of the HIP library (``pn_cross_entropy``, ``pn_adam_step``): same arithmetic as ``torch.nn.CrossEntropyLoss()``
and ``torch.optim.Adam(lr, betas, eps, weight_decay)``, ~10 us instead of ~100 us per step on the bench workload.
Class weights, ``ignore_index`` and label smoothing go through ``pn_cross_entropy_ex`` (one launch more: the weighted
mean's denominator, formed on the device).  The optimizer's options -- amsgrad, decoupled weight decay (AdamW),
gradient-norm clipping, a non-finite guard and a learning-rate schedule evaluated on the device -- go through
``pn_grad_norm`` / ``pn_adam_step_ex`` (one launch more when a norm is wanted)."""
import ctypes
import math
import struct

import torch

from . import _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        if not logits.is_cuda:
            raise RuntimeError("pathnet_amd.cross_entropy: logits must be on the GPU (there is no CPU fallback)")
        lib = _lib.load()
        x = logits.contiguous().float()
        t = target.to(device=x.device, dtype=torch.int64).contiguous()
        if x.dim() != 2 or t.shape != (x.shape[0],):
            raise ValueError("cross_entropy: logits [rows, classes] and int targets [rows] expected")
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        g = torch.empty_like(x) if logits.requires_grad else None
        with torch.cuda.device(x.device):
            _lib.check(lib.pn_cross_entropy(_lib.ptr(x), _lib.ptr(t), x.shape[0], x.shape[1], _lib.ptr(loss),
                                            _lib.ptr(g), _stream()))
        ctx.g = g
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        if ctx.g is None:
            return None, None
        # loss.backward() hands a freshly filled ones tensor down and costs a multiply by it: two launches for nothing.
        # optim.backward(loss) passes the cached tensor of `unit()` instead, recognised here by identity
        one = _UNIT.get(grad_out.device)
        if one is not None and grad_out.data_ptr() == one.data_ptr():
            return ctx.g, None
        return ctx.g * grad_out, None


class _CrossEntropyEx(torch.autograd.Function):
    """pn_cross_entropy_ex: the loss with the options of `loss_fn` (a CrossEntropyLoss)"""

    @staticmethod
    def forward(ctx, logits, target, loss_fn):
        if not logits.is_cuda:
            raise RuntimeError("pathnet_amd.cross_entropy: logits must be on the GPU (there is no CPU fallback)")
        lib = _lib.load()
        x = logits.contiguous().float()
        t = target.to(device=x.device, dtype=torch.int64).contiguous()
        if x.dim() != 2 or t.shape != (x.shape[0],):
            raise ValueError("cross_entropy: logits [rows, classes] and int targets [rows] expected")
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        g = torch.empty_like(x) if logits.requires_grad else None
        with torch.cuda.device(x.device):
            spec, keep = loss_fn.spec(x.device, x.shape[1], 1.0)
            _lib.check(lib.pn_cross_entropy_ex(_lib.ptr(x), _lib.ptr(t), x.shape[0], x.shape[1], ctypes.byref(spec),
                                               _lib.ptr(loss), _lib.ptr(g), _stream()))
        ctx.g = g
        ctx.keep = keep
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        if ctx.g is None:
            return None, None, None
        one = _UNIT.get(grad_out.device)
        if one is not None and grad_out.data_ptr() == one.data_ptr():
            return ctx.g, None, None
        return ctx.g * grad_out, None, None


_UNIT = {}


def unit(device):
    """the cached scalar 1.0 on `device` that `backward(loss)` seeds autograd with"""
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    t = _UNIT.get(dev)
    if t is None:
        t = _UNIT[dev] = torch.ones((), dtype=torch.float32, device=dev)
    return t


def backward(loss):
    """``loss.backward()`` for a scalar loss of this module's cross entropy without the two launches autograd spends on the
    seed gradient (a ones_like fill, and the multiply by it in the loss's backward): the seed is a cached tensor that the
    loss recognises.  Same gradients, bit for bit."""
    loss.backward(unit(loss.device))


def cross_entropy(logits, target, weight=None, ignore_index=None, label_smoothing=0.0, reduction="mean"):
    """Softmax cross entropy, = ``torch.nn.functional.cross_entropy(logits, target, weight, ignore_index=...,
    label_smoothing=..., reduction=...)`` -- see CrossEntropyLoss for the options and the two differences.  With every
    option at its default this is the plain mean (pn_cross_entropy), as it always was."""
    if weight is None and ignore_index is None and label_smoothing == 0.0 and reduction == "mean":
        return _CrossEntropy.apply(logits, target)
    return CrossEntropyLoss(weight, ignore_index, label_smoothing, reduction)(logits, target)


def balanced_class_weight(target, num_classes, ignore_index=None):
    """scikit-learn's "balanced" class weights of a target tensor: ``n_kept / (num_classes * count_c)``, where a row is
    kept when its target is a class in ``[0, num_classes)`` and not ``ignore_index``; a class without a kept row gets
    weight 0.  fp32 [num_classes] on the target's device; nothing is read back."""
    t = torch.as_tensor(target).reshape(-1).to(torch.int64)
    kept = (t >= 0) & (t < num_classes)
    if ignore_index is not None:
        kept = kept & (t != int(ignore_index))
    count = torch.zeros(num_classes, dtype=torch.float32, device=t.device)
    count.index_add_(0, torch.where(kept, t, torch.zeros_like(t)), kept.to(torch.float32))
    w = count.sum() / (float(num_classes) * count)
    return torch.where(count > 0, w, torch.zeros_like(w))


class CrossEntropyLoss(torch.nn.Module):
    """``torch.nn.CrossEntropyLoss(weight, ignore_index=..., label_smoothing=..., reduction="mean" | "sum")`` for int64
    class targets (include/pathnet_hip.h, pn_loss_spec, has the formulas).

    ``ignore_index=None`` is the default and means NO ignore value -- pass ``-100`` for torch's default.  A bare
    ``CrossEntropyLoss()`` is the reference's (PathNet_run.py:297): the plain mean through ``pn_cross_entropy``, and a
    target outside ``[0, classes)`` -- the ``-1`` of an unlabelled node -- poisons the loss (NaN, so the mistake cannot go
    unnoticed) and gets a zero gradient row.  With ``ignore_index=-1`` those rows are dropped instead: they add nothing to
    the loss, to the weighted mean's denominator or to any gradient, and their logits are not looked at.

    Two differences from torch, after this library's rule that every gradient stays finite: a target outside
    ``[0, classes)`` that is NOT the ignore value still gives a NaN loss and a zero gradient row (torch raises or reads out
    of bounds); and when the mean's denominator is zero -- every row ignored, or only zero-weight classes among the kept
    rows -- the loss is NaN and every gradient is zero (torch: NaN gradients in the zero-weight case).

    The denominator depends on the targets and is formed on the device; nothing is read back, so a captured step may be
    replayed with targets whose ignored count differs.  ``forward_loss(..., loss=this)`` of the aggregators takes the same
    options on every route.  Not covered: ``reduction="none"`` and probability targets."""

    def __init__(self, weight=None, ignore_index=None, label_smoothing=0.0, reduction="mean"):
        super().__init__()
        if reduction not in ("mean", "sum"):
            raise ValueError("CrossEntropyLoss: reduction %r (mean | sum)" % (reduction,))
        if not 0.0 <= float(label_smoothing) <= 1.0:
            raise ValueError("CrossEntropyLoss: label_smoothing %r outside [0, 1]" % (label_smoothing,))
        self.register_buffer("weight", None if weight is None else torch.as_tensor(weight, dtype=torch.float32).detach())
        self.ignore_index = None if ignore_index is None else int(ignore_index)
        self.label_smoothing = float(label_smoothing)
        self.reduction = reduction
        self._weight_on = None      # (device, source tensor, its version, contiguous fp32 copy on the device)

    @property
    def has_options(self):
        return (self.weight is not None or self.ignore_index is not None or self.label_smoothing != 0.0 or
                self.reduction != "mean")

    def _device_weight(self, device):
        w = self.weight
        if w is None:
            return None
        if w.device == device and w.is_contiguous():
            return w
        hit = self._weight_on
        if hit is None or hit[0] != device or hit[1] is not w or hit[2] != w._version:
            hit = self._weight_on = (device, w, w._version, w.to(device).contiguous())
        return hit[3]

    def spec(self, device, classes, grad_scale=1.0):
        """(pn_loss_spec, tensors it points to) for a call on `device` with `classes` classes: keep the second alive until
        the call's kernels have run (under capture: allocate it inside the capture)."""
        device = torch.device(device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        w = self._device_weight(device)
        if w is not None and tuple(w.shape) != (classes,):
            raise ValueError("CrossEntropyLoss: %d class weights for %d classes" % (w.numel(), classes))
        mean = self.reduction == "mean"
        denom = torch.empty(1, dtype=torch.float32, device=device) if mean else None
        spec = _lib.LossSpec(_lib.ptr(w), self.ignore_index if self.ignore_index is not None else 0,
                             0 if self.ignore_index is None else 1, self.label_smoothing,
                             _lib.LOSS_MEAN if mean else _lib.LOSS_SUM, float(grad_scale), _lib.ptr(denom), 0)
        return spec, (w, denom)

    def forward(self, logits, target):
        if not self.has_options:
            return _CrossEntropy.apply(logits, target)
        return _CrossEntropyEx.apply(logits, target, self)


def _f32(x):
    """the float a hyper-parameter becomes when it crosses the C ABI, as a Python double"""
    return struct.unpack("f", struct.pack("f", float(x)))[0]


class LRSchedule:
    """A learning-rate schedule that the optimizer's kernel evaluates ON THE DEVICE from the step count (so a step captured
    in a hipGraph replays with the learning rate of its own step).  With e = step - 1 (step counts from 1):

        lr_now = lr * warm(e) * decay(max(e - warmup_steps, 0))
        warm(e) = start_factor + (1 - start_factor) * min(e, warmup_steps) / warmup_steps        (1 without warm-up)

    kind        decay(e)                                                                 torch
    constant    1                                                                        (LinearLR for the warm-up)
    step        gamma ** (e // step_size)                                                StepLR
    exponential gamma ** e                                                               ExponentialLR
    cosine      (lr_min + (lr - lr_min) * (1 + cos(pi * min(e, t_max) / t_max)) / 2) / lr   CosineAnnealingLR, closed form

    The cosine stays at lr_min after t_max; torch's recursion turns upwards again there, this does not.  A value object:
    `lr_at(base_lr, step)` is the host mirror in Python doubles -- nothing is read back from the device."""

    KINDS = {"constant": _lib.LR_CONSTANT, "step": _lib.LR_STEP, "exponential": _lib.LR_EXPONENTIAL, "cosine": _lib.LR_COSINE}

    def __init__(self, kind="constant", warmup_steps=0, start_factor=1.0 / 3.0, step_size=None, gamma=None, t_max=None,
                 lr_min=0.0):
        if kind not in self.KINDS:
            raise ValueError("LRSchedule: kind %r (constant | step | exponential | cosine)" % (kind,))
        if int(warmup_steps) != warmup_steps or warmup_steps < 0:
            raise ValueError("LRSchedule: warmup_steps %r" % (warmup_steps,))
        if not 0.0 <= float(start_factor) <= 1.0:
            raise ValueError("LRSchedule: start_factor %r outside [0, 1]" % (start_factor,))
        if kind == "step" and (step_size is None or int(step_size) != step_size or step_size < 1):
            raise ValueError("LRSchedule: step needs an integer step_size >= 1 (got %r)" % (step_size,))
        if kind in ("step", "exponential") and (gamma is None or not 0.0 < float(gamma) < math.inf):
            raise ValueError("LRSchedule: %s needs a finite gamma > 0 (got %r)" % (kind, gamma))
        if kind == "cosine" and (t_max is None or int(t_max) != t_max or t_max < 1):
            raise ValueError("LRSchedule: cosine needs an integer t_max >= 1 (got %r)" % (t_max,))
        if not 0.0 <= float(lr_min) < math.inf:
            raise ValueError("LRSchedule: lr_min %r" % (lr_min,))
        self.kind = kind
        self.warmup_steps = int(warmup_steps)
        self.start_factor = float(start_factor)
        self.step_size = int(step_size) if step_size is not None else 1
        self.gamma = float(gamma) if gamma is not None else 1.0
        self.t_max = int(t_max) if t_max is not None else 1
        self.lr_min = float(lr_min)

    def check_lr(self, lr):
        if self.kind == "cosine" and self.lr_min > _f32(lr):
            raise ValueError("LRSchedule: lr_min %r above the learning rate %r" % (self.lr_min, lr))

    def lr_at(self, base_lr, step):
        """the learning rate of step `step` (from 1) for the base rate `base_lr` (as the kernel sees it: rounded to fp32)"""
        lr = _f32(base_lr)
        e = int(step) - 1
        if e < 0:
            raise ValueError("LRSchedule.lr_at: step counts from 1")
        warm = 1.0
        if self.warmup_steps > 0:
            warm = self.start_factor + (1.0 - self.start_factor) * float(min(e, self.warmup_steps)) / float(self.warmup_steps)
        d = max(e - self.warmup_steps, 0)
        decay = 1.0
        if self.kind == "step":
            decay = self.gamma ** float(d // self.step_size)
        elif self.kind == "exponential":
            decay = self.gamma ** float(d)
        elif self.kind == "cosine" and lr > 0.0:
            c = float(min(d, self.t_max)) / float(self.t_max)
            decay = (self.lr_min + (lr - self.lr_min) * (1.0 + math.cos(math.pi * c)) / 2.0) / lr
        return lr * warm * decay

    def fill(self, spec):
        spec.schedule = self.KINDS[self.kind]
        spec.warmup_steps, spec.start_factor = self.warmup_steps, self.start_factor
        spec.step_size, spec.gamma, spec.t_max, spec.lr_min = self.step_size, self.gamma, self.t_max, self.lr_min

    def __repr__(self):
        return ("LRSchedule(%r, warmup_steps=%d, start_factor=%r, step_size=%d, gamma=%r, t_max=%d, lr_min=%r)"
                % (self.kind, self.warmup_steps, self.start_factor, self.step_size, self.gamma, self.t_max, self.lr_min))


def _adam_tensors(items):
    arr = (_lib.AdamTensor * max(len(items), 1))()
    for i, (p, g, st) in enumerate(items):
        arr[i] = _lib.AdamTensor(p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr() if st else None,
                                 st["exp_avg_sq"].data_ptr() if st else None, p.numel())
    return arr


def _optim_state(device, n_tensors, total_elements):
    """a zeroed pn_optim state buffer as float64 words: [grad_norm, lr, (clip_coef, n_partials), skipped, partials ...]"""
    nbytes = ctypes.c_int64()
    _lib.check(_lib.load().pn_optim_state_bytes(total_elements, n_tensors, ctypes.byref(nbytes)))
    return torch.zeros((nbytes.value + 7) // 8, dtype=torch.float64, device=device)


class Adam(torch.optim.Optimizer):
    """Drop-in for ``torch.optim.Adam(params, lr, betas, eps, weight_decay)`` (no maximize): one launch per step over all
    parameters.  State keys match torch's (``step``, ``exp_avg``, ``exp_avg_sq``, with amsgrad ``max_exp_avg_sq``), and
    ``load_state_dict`` takes the state of a torch.optim.Adam / AdamW.

    With no option set ``step()`` is ``pn_adam_step`` / ``pn_adam_step_advance``, as it always was.  The options
    (``pn_adam_step_ex``, include/pathnet_hip.h has the order of operations):

    amsgrad                    ``torch.optim.Adam(amsgrad=True)``
    decoupled_weight_decay     ``torch.optim.AdamW``: ``p *= 1 - lr_now * weight_decay`` instead of ``g += weight_decay * p``
    max_grad_norm              ``torch.nn.utils.clip_grad_norm_(all parameters of all groups, max_grad_norm)`` before the
                               update, fused into it: one launch more for the norm, taken once per ``step()`` over every
                               group's gradients; the gradients themselves are NOT modified
    skip_nonfinite             the non-finite guard without clipping (clipping always has it): when the gradients' sum of
                               squares is inf or NaN the step updates nothing -- parameters and state keep their bits --
                               and ``skipped_steps`` goes up.  The step count still advances: a skipped step uses up its
                               place in the schedule and in the bias corrections.
    schedule                   an LRSchedule, evaluated on the device from the step count

    ``last_grad_norm`` (float64; NaN when no norm is taken), ``last_lr`` (float64), ``last_clip_coef`` (float32) and
    ``skipped_steps`` (int64) are 0-d VIEWS of the optimizer's device state buffer, None before the first ``step()``:
    reading one (``.item()``) is the caller's synchronisation, the library reads nothing back.  The buffer is allocated at
    the first ``step()`` and kept, so a step captured after a warm-up step stays valid."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step_state=None, *, amsgrad=False,
                 decoupled_weight_decay=False, max_grad_norm=None, skip_nonfinite=False, schedule=None):
        """step_state (StepState): the step count of the bias corrections is read from device memory when the kernel runs
        (a step captured in a hipGraph can be replayed); state["step"] then only counts the Python-side calls."""
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("Adam: invalid hyper-parameter")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("Adam: max_grad_norm %r (a positive number, inf for the non-finite guard alone)" % (max_grad_norm,))
        if schedule is not None:
            if not isinstance(schedule, LRSchedule):
                raise ValueError("Adam: schedule must be an LRSchedule")
            schedule.check_lr(lr)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.step_state = step_state
        self.amsgrad = bool(amsgrad)
        self.decoupled_weight_decay = bool(decoupled_weight_decay)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.schedule = schedule
        self._optim_state = None        # the device state buffer of the option route (float64 words)

    @property
    def has_options(self):
        return (self.amsgrad or self.decoupled_weight_decay or self.max_grad_norm is not None or self.skip_nonfinite or
                self.schedule is not None)

    @property
    def last_grad_norm(self):
        return None if self._optim_state is None else self._optim_state[0]

    @property
    def last_lr(self):
        return None if self._optim_state is None else self._optim_state[1]

    @property
    def last_clip_coef(self):
        return None if self._optim_state is None else self._optim_state[2:3].view(torch.float32)[0]

    @property
    def skipped_steps(self):
        return None if self._optim_state is None else self._optim_state[3:4].view(torch.int64)[0]

    def load_state_dict(self, state_dict):
        """torch's, after which a ``step`` that arrived as a tensor (torch.optim's own state) is a Python int again"""
        super().load_state_dict(state_dict)
        for st in self.state.values():
            if torch.is_tensor(st.get("step")):
                st["step"] = int(st["step"].item())

    def _collect(self, group):
        todo = []
        for p in group["params"]:
            if p.grad is None:
                continue
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("pathnet_amd.Adam: contiguous fp32 GPU parameters only")
            st = self.state[p]
            if not st:
                st["step"] = 0
                st["exp_avg"] = torch.zeros_like(p)
                st["exp_avg_sq"] = torch.zeros_like(p)
            if self.amsgrad and "max_exp_avg_sq" not in st:
                st["max_exp_avg_sq"] = torch.zeros_like(p)
            st["step"] += 1
            todo.append((p, p.grad.contiguous(), st))
        return todo

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        if self.has_options:
            self._step_with_options(lib)
            return loss
        for group in self.param_groups:
            todo = self._collect(group)
            # tensors that have taken the same number of steps share a launch (normally: all of them)
            by_step = {}
            for item in todo:
                by_step.setdefault(item[2]["step"], []).append(item)
            groups_left = len(by_step)
            for step, items in by_step.items():
                groups_left -= 1
                arr = _adam_tensors(items)
                ss = self.step_state
                with torch.cuda.device(items[0][0].device):
                    if ss is not None and ss.advance_in_adam and groups_left == 0 and group is self.param_groups[-1]:
                        # the optimizer's last launch of the step moves the step state on: the next StepState.advance() is free
                        _lib.check(lib.pn_adam_step_advance(arr, len(items), group["lr"], group["betas"][0], group["betas"][1],
                                                            group["eps"], group["weight_decay"], ss.ptr(), _stream()))
                        ss._advanced_by_adam = True
                    else:
                        _lib.check(lib.pn_adam_step(arr, len(items), group["lr"], group["betas"][0], group["betas"][1],
                                                    group["eps"], group["weight_decay"], step,
                                                    ss.ptr() if ss is not None else None, _stream()))
                # the kernel wrote through raw pointers: tell autograd's version counters, which is what everything that
                # caches a function of the parameters keys on (the modules' reuse_tables, dist.ShardedAggregator.begin_step) --
                # torch.optim.Adam's in-place ops bump them as a matter of course.  No launch.
                for p, _, _ in items:
                    torch.autograd.graph.increment_version(p)
        return loss

    def _step_with_options(self, lib):
        """pn_grad_norm once over every group's gradients (when a norm is wanted), then pn_adam_step_ex per group"""
        work = []       # (group, step, items): the launches of this step, in order
        for group in self.param_groups:
            by_step = {}
            for item in self._collect(group):
                by_step.setdefault(item[2]["step"], []).append(item)
            work += [(group, step, items) for step, items in by_step.items()]
        everything = [item for _, _, items in work for item in items]
        if not everything:
            return
        device = everything[0][0].device
        if any(p.device != device for p, _, _ in everything):
            raise RuntimeError("pathnet_amd.Adam: the gradient norm is global -- every parameter on one device")
        if self._optim_state is None:
            # sized once, for every parameter of every group: a later step with more gradients than the first still fits
            every = [p for group in self.param_groups for p in group["params"]]
            self._optim_state = _optim_state(device, len(every), sum(p.numel() for p in every))
        state = _lib.ptr(self._optim_state)
        max_norm = self.max_grad_norm if self.max_grad_norm is not None else (math.inf if self.skip_nonfinite else 0.0)
        flags = ((_lib.OPTIM_DECOUPLED_WD if self.decoupled_weight_decay else 0) | (_lib.OPTIM_AMSGRAD if self.amsgrad else 0))
        ss = self.step_state
        with torch.cuda.device(device):
            if max_norm != 0.0:
                _lib.check(lib.pn_grad_norm(_adam_tensors(everything), len(everything), state, _stream()))
            for k, (group, step, items) in enumerate(work):
                spec = _lib.OptimSpec(flags=flags | (_lib.OPTIM_NO_REPORT if k else 0), max_grad_norm=max_norm,
                                      start_factor=1.0, step_size=1, gamma=1.0, t_max=1)
                if self.schedule is not None:
                    self.schedule.check_lr(group["lr"])
                    self.schedule.fill(spec)
                arr = (_lib.AdamTensorEx * len(items))()
                for i, (p, g, st) in enumerate(items):
                    vmax = st["max_exp_avg_sq"].data_ptr() if self.amsgrad else None
                    arr[i] = _lib.AdamTensorEx(p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(),
                                               st["exp_avg_sq"].data_ptr(), vmax, p.numel())
                hyper = (group["lr"], group["betas"][0], group["betas"][1], group["eps"], group["weight_decay"])
                if ss is not None and ss.advance_in_adam and k == len(work) - 1:
                    _lib.check(lib.pn_adam_step_ex_advance(arr, len(items), *hyper, ctypes.byref(spec), state, ss.ptr(),
                                                           _stream()))
                    ss._advanced_by_adam = True
                else:
                    _lib.check(lib.pn_adam_step_ex(arr, len(items), *hyper, ctypes.byref(spec), state, step,
                                                   ss.ptr() if ss is not None else None, _stream()))
                for p, _, _ in items:       # (see step(): the version counters of what the kernel wrote)
                    torch.autograd.graph.increment_version(p)


class AdamW(Adam):
    """``torch.optim.AdamW``: pathnet_amd.Adam with decoupled weight decay and torch's default ``weight_decay=1e-2``;
    every other option as there."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, step_state=None, *, amsgrad=False,
                 max_grad_norm=None, skip_nonfinite=False, schedule=None):
        super().__init__(params, lr, betas, eps, weight_decay, step_state, amsgrad=amsgrad, decoupled_weight_decay=True,
                         max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, schedule=schedule)


def clip_grad_norm_(parameters, max_norm):
    """``torch.nn.utils.clip_grad_norm_(parameters, max_norm)`` (the 2-norm) in place, in two launches and without a host
    read: the sum of squares in float64, then ``grad *= min(1, max_norm / (norm + 1e-6))``.  Returns the norm before
    clipping as a 0-d float64 device tensor.  A non-finite norm leaves the gradients as they are (torch turns all of them
    into NaN): test the returned norm, or let the optimizer's ``skip_nonfinite`` skip the step."""
    if not float(max_norm) > 0.0:
        raise ValueError("clip_grad_norm_: max_norm %r" % (max_norm,))
    if torch.is_tensor(parameters):
        parameters = [parameters]
    items = []
    for p in parameters:
        g = p.grad
        if g is None:
            continue
        if not g.is_cuda or g.dtype != torch.float32 or not g.is_contiguous():
            raise RuntimeError("pathnet_amd.clip_grad_norm_: contiguous fp32 GPU gradients only")
        items.append((g, g, None))
    if not items:
        return torch.zeros((), dtype=torch.float64)
    device = items[0][0].device
    if any(g.device != device for g, _, _ in items):
        raise RuntimeError("pathnet_amd.clip_grad_norm_: every gradient on one device")
    state = _optim_state(device, len(items), sum(g.numel() for g, _, _ in items))
    with torch.cuda.device(device):
        _lib.check(_lib.load().pn_clip_grad_norm(_adam_tensors(items), len(items), float(max_norm), _lib.ptr(state),
                                                 _stream()))
    return state[0]


class StepState:
    """struct pn_step_state in device memory: {epoch, seed, adam_step} of the current training step, read by the sampler,
    the aggregator's dropout and Adam WHEN THEIR KERNELS RUN -- so a whole step (sample -> forward -> loss -> backward ->
    Adam) captured into a hipGraph (torch.cuda.CUDAGraph) replays with a new epoch / seed / step count each time.
    ``advance()`` is the first launch of a step: epoch += 1, adam_step += 1, seed = splitmix64(seed).
    advance_in_adam (round 6): pathnet_amd.Adam's last launch of a step performs the advance for the NEXT step
    (pn_adam_step_advance), and the ``advance()`` that follows it launches nothing -- one launch less on the step's critical
    path; every ``advance()`` still stands for exactly one advance of the state."""

    def __init__(self, device="cuda", seed=0, first_epoch=0, advance_in_adam=False):
        dev = torch.device(device)
        self.t = torch.tensor([int(first_epoch) - 1, int(seed) & 0x7FFFFFFFFFFFFFFF, 0, 0], dtype=torch.int64, device=dev)
        self.advance_in_adam = bool(advance_in_adam)
        self._advanced_by_adam = False

    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def advance(self):
        if self._advanced_by_adam:      # the optimizer step before this one has already moved the state
            self._advanced_by_adam = False
            return
        with torch.cuda.device(self.t.device):
            _lib.check(_lib.load().pn_step_state_advance(self.ptr(), _lib.stream_ptr(self.t.device)))

    def values(self):
        e, s, a, _ = self.t.tolist()
        return {"epoch": e, "seed": s & 0xFFFFFFFFFFFFFFFF, "adam_step": a}
