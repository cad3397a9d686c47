"""Plain fp64 references of the optimizer's options -- pn_grad_norm, pn_adam_step_ex / pn_adam_step_ex_advance and
pn_clip_grad_norm (pn_optim.hip) -- their rounding bounds, and the case tables of tests/test_gpu_optim_options.py.
torch in float64 and Python numbers only: no library code, no GPU.  tests/test_optim_options_host.py holds the references
to torch's own float64 implementations and the tables to the dispatch constants in the source.  Style, `f32` and `U` are
optim_ref's, and with every option off adam_ex_ref IS optim_ref.adam_ref, bound included.

The rounding bound of adam_ex_ref
---------------------------------
optim_ref's docstring has the rules (u = 2^-24 per fp32 operation on the absolute values of its terms, sqrtf and the
division 2 u, errors carried through the derivatives) and the lines of the option-less update.  The options change them
as follows; the names are those of adam_ex_kernel.

    coef = (float) min(1, max_norm / (norm + 1e-6))     formed in double from the fp64 norm: the conversion (u), the norm's
                                                        relative error N (norm_ref) and three double operations (2^-50):
                                                        C = u + N + 2^-50, relative.  No clipping: coef is the constant 1.0f
                                                        and the product below is exact (C = 0, and its u is not charged).
    gc = coef grad               1 product              E_gc = (C + u) |gc|                      (0 without clipping)
    L2:        g = gc + wd p     1 product, 1 sum       E_g  = E_gc + u (|gc| + 2 |wd p|)
    decoupled: g = gc                                   E_g  = E_gc
               keep = (float)(1 - lr_now wd)            the conversion (u); the double arithmetic behind it moves keep by
                                                        2^-40 lr_now wd at most (lr_now's own 2^-40, below)
               pd = p keep       1 product              E_pd = 2 u |pd| + 2^-40 lr_now wd |p|    (the "one product and one
                                                        subtraction on p": the subtraction is the double one inside keep)
    m', v'                       as optim_ref, with G = |gc| + |wd p| (L2) or |gc| (decoupled) and the E_g above
    amsgrad: vd = max(vmax, v')  no rounding: max is exact, and 1-Lipschitz in each argument, so
                                                        E_vd = max(E_vmax, E_v') elementwise; vd and E_vd stand where v' and
                                                        E_v' stood in the denominator's line
    c1 = (float)(lr_now / (1 - b1^step))                lr_now replaces lr.  It is formed in double on the device (pow, cospi,
                                                        a dozen operations at most: relative 2^-48 or better where the
                                                        schedule's value still matters) -- inside the 2^-40 optim_ref
                                                        already grants c1.
    p' = pd - s  (pd = p in L2 mode)                    E_p  = E_s + u |p'| + E_pd

In a trajectory (err=) the errors of the inputs pass through the same derivatives as in optim_ref: wd E_p into g (L2
only), keep E_p into pd, b1 E_m, b2 E_v, and E_vmax through the max.  A skipped step (non-finite norm) changes nothing:
the caller carries values and bounds over unchanged.

The bound of norm_ref
---------------------
grad_sumsq_kernel squares in double -- exact, the square of a 24-bit significand has 48 bits -- and adds in double:
a thread's elements in order, 6 butterfly steps, 4 wavefronts, and the consumer sums the partials the same way (a
thread's partials in order, 6 butterfly steps, 4 wavefronts).  No sum passes through more than n + 64 additions (a
thread sees fewer than n elements, then fewer than n partials), each relative 2^-53 of a sum of non-negative terms: the sum of squares is
within (n + 64) 2^-53, relative.  The square root halves that and adds its own 2^-53; (n + 64) 2^-53 is kept for the
norm as well.  The reference adds the squares with math.fsum (correctly rounded)."""
import itertools
import math

import torch

import optim_ref as R
from optim_ref import U, f32

# dispatch constants of pn_optim.hip (held to the source by tests/test_optim_options_host.py)
OPT_CHUNK = 2048
OPT_THREADS = 256
OPT_GRID_CAP = 256
MAX_TENSORS = 32


# ------------------------------------------------------------------------------------------------
# learning-rate schedule
# ------------------------------------------------------------------------------------------------
def lr_ref(base_lr, step, kind="constant", warmup_steps=0, start_factor=1.0 / 3.0, step_size=1, gamma=1.0, t_max=1,
           lr_min=0.0):
    """lr_now of step `step` (from 1) in Python doubles, at the fp32-rounded base rate:
    lr * warm(e) * decay(max(e - warmup_steps, 0)), e = step - 1"""
    lr = f32(base_lr)
    e = int(step) - 1
    assert e >= 0
    warm = 1.0
    if warmup_steps > 0:
        warm = start_factor + (1.0 - start_factor) * min(e, warmup_steps) / warmup_steps
    d = max(e - warmup_steps, 0)
    if kind == "constant":
        decay = 1.0
    elif kind == "step":
        decay = math.pow(gamma, d // step_size)
    elif kind == "exponential":
        decay = math.pow(gamma, d)
    elif kind == "cosine":
        decay = (lr_min + (lr - lr_min) * (1.0 + math.cos(math.pi * min(d, t_max) / t_max)) / 2.0) / lr
    else:
        raise ValueError(kind)
    return lr * warm * decay


# ------------------------------------------------------------------------------------------------
# gradient norm and clip coefficient
# ------------------------------------------------------------------------------------------------
def norm_ref(grads):
    """the 2-norm over a list of tensors in float64 -> (norm, N): N the relative bound of the kernel's norm (docstring)"""
    n = sum(g.numel() for g in grads)
    squares = []
    for g in grads:
        squares += (g.detach().double().reshape(-1) ** 2).tolist()
    return math.sqrt(math.fsum(squares)), (n + 64) * 2.0 ** -53


def coef_ref(norm, max_norm, norm_rel=0.0):
    """clip_grad_norm_'s coefficient min(1, max_norm / (norm + 1e-6)) at the fp32-rounded max_norm -> (coef, C): C the
    relative bound of the kernel's float coefficient.  max_norm None or inf: (1, 0), the product by it is exact."""
    if max_norm is None or math.isinf(max_norm):
        return 1.0, 0.0
    return min(1.0, f32(max_norm) / (norm + 1e-6)), U + norm_rel + 2.0 ** -50


# ------------------------------------------------------------------------------------------------
# the update
# ------------------------------------------------------------------------------------------------
def adam_ex_ref(p, g, m, v, vmax, step, lr, b1, b2, eps, wd, *, decoupled=False, amsgrad=False, coef=1.0, coef_rel=0.0,
                lr_now=None, err=None):
    """One step of torch.optim.Adam / AdamW (decoupled) with or without amsgrad on the gradient coef * g, at the learning
    rate lr_now (None: lr), in float64 at the float32-rounded hyper-parameters
    -> ((p', m', v', vmax'), (E_p, E_m, E_v, E_vmax)): the updated tensors and the elementwise rounding bound of
    adam_ex_kernel's fp32 evaluation of each (module docstring).  vmax may be None without amsgrad (vmax' is then None and
    E_vmax zero).  coef_rel: the relative bound C of the kernel's coefficient (coef_ref), 0 = no clipping.
    err = the four bounds of the step before, for a trajectory."""
    lr, b1, b2, eps, wd = (f32(x) for x in (lr, b1, b2, eps, wd))
    lr_now = lr if lr_now is None else float(lr_now)
    p, g0, m0, v0 = (t.detach().double() for t in (p, g, m, v))
    step = int(step)
    c1 = lr_now / (1.0 - b1 ** step)
    c2 = 1.0 / math.sqrt(1.0 - b2 ** step)
    o1, o2 = 1.0 - b1, 1.0 - b2
    zero = torch.zeros_like(p)
    Ep0, Em0, Ev0, Ex0 = err if err is not None else (zero, zero, zero, zero)

    gc = coef * g0
    E_gc = (coef_rel + U) * gc.abs() if coef_rel > 0.0 else zero
    if decoupled:
        keep = 1.0 - lr_now * wd
        pd = p * keep
        gg = gc
        G = gc.abs()
        E_g = E_gc
        E_pd = 2.0 * U * pd.abs() + 2.0 ** -40 * lr_now * wd * p.abs() + abs(keep) * Ep0
    else:
        pd = p
        gg = gc + wd * p
        G = gc.abs() + (wd * p).abs() + wd * Ep0
        E_g = E_gc + U * (gc.abs() + 2.0 * (wd * p).abs()) + wd * Ep0
        E_pd = Ep0
    m1 = b1 * m0 + o1 * gg
    v1 = b2 * v0 + o2 * gg * gg
    E_m = U * (2.0 * (b1 * m0).abs() + 3.0 * o1 * G) + o1 * E_g + b1 * Em0
    E_v = U * (2.0 * b2 * v0.abs() + 4.0 * o2 * G * G) + 2.0 * o2 * G * E_g + b2 * Ev0
    if amsgrad:
        x1 = torch.maximum(vmax.detach().double(), v1)
        E_x = torch.maximum(Ex0 + zero, E_v)
        vd, E_vd = x1, E_x
    else:
        x1, E_x = None, zero
        vd, E_vd = v1, E_v
    rv = vd.sqrt()
    d = rv * c2 + eps
    q = m1 / d
    p1 = pd - c1 * q
    E_d = c2 * (rv - (vd - E_vd).clamp_min(0.0).sqrt()) + U * (5.0 * c2 * rv + eps) + 2.0 ** -40 * c2 * rv
    d_lo = (d - E_d).clamp_min(1e-300)
    E_q = 2.0 * U * q.abs() + (E_m + q.abs() * E_d) / d_lo
    E_s = c1 * ((2.0 * U + 2.0 ** -40) * q.abs() + E_q)
    E_p = E_s + U * p1.abs() + E_pd
    slack = 1.0 + 2.0 ** -10
    return (p1, m1, v1, x1), (E_p * slack, E_m * slack, E_v * slack, E_x * slack)


def adam_ex_f32(p, g, m, v, vmax, step, lr, b1, b2, eps, wd, *, decoupled=False, amsgrad=False, coef=1.0, lr_now=None):
    """adam_ex_kernel's lines in torch float32 on the CPU, one rounding per operation (no FMA), the block-uniform scalars
    formed in double and converted once -> (p', m', v', vmax') in fp32: the bound of adam_ex_ref must hold for it."""
    F = torch.float32
    lr, b1, b2, eps, wd = (f32(x) for x in (lr, b1, b2, eps, wd))
    lr_now = lr if lr_now is None else float(lr_now)
    t = lambda x: torch.tensor(x, dtype=F)      # noqa: E731  (a double, converted once)
    c1, c2 = t(lr_now / (1.0 - b1 ** int(step))), t(1.0 / math.sqrt(1.0 - b2 ** int(step)))
    p, g, m, v = (x.detach().to(F) for x in (p, g, m, v))
    g = t(coef) * g
    if decoupled:
        p = p * t(1.0 - lr_now * wd)
    else:
        g = g + t(wd) * p
    m1 = t(b1) * m + (t(1.0) - t(b1)) * g
    v1 = t(b2) * v + (t(1.0) - t(b2)) * g * g
    vd = v1
    x1 = None
    if amsgrad:
        vd = x1 = torch.maximum(vmax.detach().to(F), v1)
    p1 = p - c1 * (m1 / (vd.sqrt() * c2 + t(eps)))
    return p1, m1, v1, x1


# ------------------------------------------------------------------------------------------------
# case tables of tests/test_gpu_optim_options.py
# ------------------------------------------------------------------------------------------------
NORM_COUNTS = (1, 255, 256, 257, 2047, 2048, 2049, OPT_GRID_CAP * OPT_CHUNK + 1)    # the last: a second grid-stride pass
NORM_LIST_LENGTHS = (31, 32, 33, 65)        # tensors of 17 elements: the partials span launches past 32
NORM_ZERO_POSITIONS = ((0, 17, 2049), (17, 0, 2049), (17, 2049, 0))
HYPER = (0.005, (0.9, 0.999), 1e-8, 5e-4)   # optim_ref.ADAM_HYPER["recipe"]
CLIP_MODES = {"none": None, "active": 0.1, "inactive": 10.0}       # max_norm as a multiple of the norm
UPDATE_COMBOS = tuple(itertools.product((False, True), (False, True), sorted(CLIP_MODES)))   # decoupled, amsgrad, clip
WARMUP, T_MAX = 5, 40
SCHEDULES = {
    "constant": dict(kind="constant", warmup_steps=WARMUP, start_factor=0.25),
    "step": dict(kind="step", warmup_steps=WARMUP, start_factor=0.25, step_size=7, gamma=0.99999),
    "exponential": dict(kind="exponential", warmup_steps=WARMUP, start_factor=0.25, gamma=0.999999),
    "cosine": dict(kind="cosine", warmup_steps=WARMUP, start_factor=0.25, t_max=T_MAX, lr_min=1e-4),
}
SCHEDULE_STEPS = (1, 2, WARMUP, WARMUP + 1, T_MAX, T_MAX + 1, 10 ** 6)


def warm_state(n, seed):
    """(p, g, m, v, vmax) fp32 [n] of an optimizer some steps in: vmax >= v in places and below it in others"""
    gen = torch.Generator().manual_seed(seed)
    p, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    m = 0.1 * torch.randn(n, generator=gen)
    v = (0.1 * torch.randn(n, generator=gen)) ** 2
    vmax = v * (0.5 + torch.rand(n, generator=gen))
    return p, g, m, v, vmax


def elements_state():
    """optim_ref.adam_elements() and a running maximum beside it: above v for every other element, below it for the rest"""
    p, g, m, v = R.adam_elements()
    vmax = torch.where(torch.arange(v.numel()) % 2 == 0, v * 2.0, v * 0.5)
    return p, g, m, v, vmax
