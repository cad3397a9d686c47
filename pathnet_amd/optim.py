"""Loss and optimizer of the reference's training step (/root/reference/PathNet_run.py:295-297, :346-352) as single
launches of the HIP library (``pn_cross_entropy``, ``pn_adam_step``): same arithmetic as ``torch.nn.CrossEntropyLoss()``
and ``torch.optim.Adam(lr, betas, eps, weight_decay)``, ~10 us instead of ~100 us per step on the bench workload.
Class weights, ``ignore_index`` and label smoothing go through ``pn_cross_entropy_ex`` (one launch more: the weighted
mean's denominator, formed on the device)."""
import ctypes

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


class Adam(torch.optim.Optimizer):
    """Drop-in for ``torch.optim.Adam(params, lr, betas, eps, weight_decay)`` (no amsgrad / maximize): one launch
    per step over all parameters.  State keys match torch's (``step``, ``exp_avg``, ``exp_avg_sq``)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step_state=None):
        """step_state (StepState): the step count of the bias corrections is read from device memory when the kernel runs
        (a step captured in a hipGraph can be replayed); state["step"] then only counts the Python-side calls."""
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("Adam: invalid hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.step_state = step_state

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        for group in self.param_groups:
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
                st["step"] += 1
                todo.append((p, p.grad.contiguous(), st))
            # tensors that have taken the same number of steps share a launch (normally: all of them)
            by_step = {}
            for item in todo:
                by_step.setdefault(item[2]["step"], []).append(item)
            groups_left = len(by_step)
            for step, items in by_step.items():
                groups_left -= 1
                arr = (_lib.AdamTensor * len(items))()
                for i, (p, g, st) in enumerate(items):
                    arr[i] = _lib.AdamTensor(p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(),
                                             st["exp_avg_sq"].data_ptr(), p.numel())
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
