"""Plain fp64 reference of the cross entropy with options -- class weights, ignore_index, label smoothing, mean / sum
(pn_loss_spec, include/pathnet_hip.h) -- and the case tables of tests/test_loss_host.py and tests/test_gpu_loss_options.py.
torch in float64 from max / exp / log / sum alone: no library code, no GPU.

    p = softmax(x_r),  lp = (x - max) - log sum exp(x - max),  w = class weights (ones),  Wsum = sum_c w[c],  e = smoothing
    row r is KEPT iff its target is not the ignore value
    l_r          = kept * [ (1 - e) w[t] (-lp[t])  +  (e / C) sum_c w[c] (-lp[c]) ]
    d l_r / d x_c = kept * [ (1 - e) w[t] (p_c - [c == t])  +  (e / C) (Wsum p_c - w[c]) ]
    D            = sum over the kept rows of w[t_r]
    loss         = k * sum_r l_r,    k = grad_scale / D (mean)  or  grad_scale (sum)

which is torch.nn.functional.cross_entropy's, but for the library's two rules (every gradient stays finite):
  - a target outside [0, C) that is not the ignore value: NaN into the loss, a zero gradient row, nothing into D;
  - D == 0 under the mean: NaN loss, ZERO gradients.
Hyper-parameters cross the C ABI as floats: the smoothing, the weights and grad_scale are rounded to fp32 first
(optim_ref.f32)."""
import itertools

import torch
from optim_ref import f32


def loss_ref(x, t, weight=None, ignore_index=None, label_smoothing=0.0, reduction="mean", grad_scale=1.0,
             denominator=None, yardstick=True):
    """-> dict(loss, grad, D: the fp64 reference;  loss32, grad32: stock fp32 torch on the CPU with the same options,
    converted to float64 (None when yardstick is False, or when a target is neither a class nor the ignore value:
    torch refuses those)).  denominator: a given D (pn_loss_spec.denominator_given) instead of the targets' own."""
    x = x.detach().cpu()
    t = t.detach().cpu().long()
    rows, C = x.shape
    x64 = x.double()
    eps = f32(label_smoothing)
    gs = f32(grad_scale)
    w = torch.ones(C, dtype=torch.float64) if weight is None else weight.detach().cpu().float().double()
    ign = (t == int(ignore_index)) if ignore_index is not None else torch.zeros(rows, dtype=torch.bool)
    ok = (t >= 0) & (t < C)
    kept = ok & ~ign
    bad = ~ok & ~ign
    tc = torch.where(ok, t, torch.zeros_like(t))
    mx = x64.max(dim=1, keepdim=True).values
    ex = (x64 - mx).exp()
    s = ex.sum(dim=1, keepdim=True)
    lp = (x64 - mx) - s.log()
    p = ex / s
    ar = torch.arange(rows)
    onehot = torch.zeros_like(x64)
    onehot[ar, tc] = 1.0
    wt = w[tc]
    row = (1.0 - eps) * wt * (-lp[ar, tc]) + (eps / C) * (w[None, :] * (-lp)).sum(dim=1)
    grow = (1.0 - eps) * wt[:, None] * (p - onehot) + (eps / C) * (w.sum() * p - w[None, :])
    keptf = kept.double()
    row = torch.where(kept, row, torch.zeros_like(row))             # (an ignored row's logits may be NaN)
    grow = torch.where(kept[:, None], grow, torch.zeros_like(grow))
    D = float((wt * keptf).sum().item())
    D_used = D if denominator is None else float(denominator)
    total = float(row.sum().item())
    if reduction == "mean":
        if D_used == 0.0:
            loss, grad = float("nan"), torch.zeros_like(grow)
        else:
            loss, grad = total * gs / D_used, grow * (gs / D_used)
    elif reduction == "sum":
        loss, grad = total * gs, grow * gs
    else:
        raise ValueError(reduction)
    if bool(bad.any()):
        loss = float("nan")
    res = {"loss": loss, "grad": grad, "D": D, "loss32": None, "grad32": None}
    if yardstick and not bool(bad.any()) and denominator is None:
        x32 = x.float().clone()
        x32[ign] = torch.nan_to_num(x32[ign], nan=0.0)      # (torch reads ignored rows too: NaN * 0)
        x32.requires_grad_(True)
        ii = int(ignore_index) if ignore_index is not None else -(10 ** 6)
        l32 = torch.nn.functional.cross_entropy(x32, t, weight=None if weight is None else weight.detach().cpu().float(),
                                                ignore_index=ii, label_smoothing=eps, reduction=reduction)
        l32 = l32 * torch.tensor(gs, dtype=torch.float32)
        l32.backward()
        res["loss32"], res["grad32"] = float(l32.item()), x32.grad.double()
    return res


def loss_bounds(ref):
    """(loss bound, gradient bound) of optim_ref.ce_bounds: as close to fp64 as fp32 torch up to the factor 8, with the
    floor 2e-6 of the value's own scale"""
    l64, g64 = ref["loss"], ref["grad"]
    lb = max(8.0 * abs(ref["loss32"] - l64), 2e-6 * max(1.0, abs(l64)))
    gb = max(8.0 * (ref["grad32"] - g64).abs().max().item(), 2e-6 * g64.abs().max().item())
    return lb, gb


# ------------------------------------------------------------------------------------------------
# case tables
# ------------------------------------------------------------------------------------------------
HOST_CLASSES = (1, 2, 7, 65)
HOST_WEIGHTS = ("none", "random", "zero")           # zero: random with one class's weight 0
HOST_IGNORE = ("none", -100, -1, "class")           # class: a valid class id (C // 2)
HOST_SMOOTHING = (0.0, 0.1, 1.0)
HOST_REDUCTIONS = ("mean", "sum")

GPU_ROWS = (1, 63, 65, 1025, 32768, 32769)          # the one-workgroup line of launch_cross_entropy and its neighbours
GPU_CLASSES = (1, 2, 65, 300)                       # at 33 rows
# every option singly, and all together: (weights, ignore, smoothing, reduction)
GPU_OPTIONS = {
    "weight": ("random", "none", 0.0, "mean"),
    "zero_weight": ("zero", "none", 0.0, "mean"),
    "ignore-1": ("none", -1, 0.0, "mean"),
    "ignore-100": ("none", -100, 0.0, "mean"),
    "ignore_class": ("none", "class", 0.0, "mean"),
    "smooth0.1": ("none", "none", 0.1, "mean"),
    "smooth1": ("none", "none", 1.0, "mean"),
    "sum": ("none", "none", 0.0, "sum"),
    "all": ("zero", -1, 0.1, "mean"),
    "all_sum": ("random", "class", 0.1, "sum"),
}


def host_cases():
    return itertools.product(HOST_WEIGHTS, HOST_IGNORE, HOST_SMOOTHING)


def make_case(rows, C, weights, ignore, seed=0, spread=3.0):
    """(x fp32 [rows, C], t int64 [rows], weight fp32 [C] or None, ignore_index or None): about a third of the rows carry
    the ignore value when it is no class; with a class as the ignore value that class's rows are the ignored ones"""
    g = torch.Generator().manual_seed(1000 * seed + 17 * rows + C)
    x = (torch.randn(rows, C, generator=g) * spread).float()
    t = torch.randint(0, C, (rows,), generator=g)
    w = None
    if weights != "none":
        w = (torch.rand(C, generator=g) * 2.0 + 0.25).float()
        if weights == "zero":
            w[C // 3] = 0.0
    ii = None
    if ignore == "class":
        ii = C // 2
    elif ignore != "none":
        ii = int(ignore)
        drop = torch.rand(rows, generator=g) < 1.0 / 3.0
        t = torch.where(drop, torch.full_like(t, ii), t)
    return x, t, w, ii
