"""Plain fp64 references of the launches that close a training step -- pn_cross_entropy, pn_adam_step /
pn_adam_step_advance (pn_train.hip) and the step-state advance (pn_context.hip) -- and the case tables their GPU tests
run (tests/test_gpu_loss_adam.py).  torch in float64 and Python integers only: no library code, no GPU.
tests/test_optim_host.py holds the references to torch's own float64 implementations and the tables to the dispatch
constants in the sources.

The rounding bound of adam_ref
------------------------------
u = 2^-24.  Every fp32 operation of adam_kernel is charged u times the absolute values of its operands' terms (a sum:
u (|a| + |b|), a product: u |a b|), sqrtf and the division 2 u, and an error that an operand already carries is passed
on through the operation's derivative.  With g0, p, m0, v0 the kernel's inputs, G = |g0| + |wd p| (>= |g|), o1 = 1 - b1,
o2 = 1 - b2, the kernel's lines give, operation by operation:

    g  = g0 + wd p                 1 product, 1 sum                        E_g = u (|g0| + 2 |wd p|)
    m' = b1 m0 + (1.0f - b1) g     1.0f - b1 (1), 2 products, 1 sum        E_m = u (2 |b1 m0| + 3 o1 G) + o1 E_g
    v' = b2 v0 + (1.0f - b2) g g   1.0f - b2 (1), 3 products, 1 sum        E_v = u (2 b2 v0 + 4 o2 G^2) + 2 o2 G E_g
    d  = sqrtf(v') c2 + eps        sqrtf (2), (float) c2 (1), 1 product,   E_d = c2 (sqrt(v') - sqrt(max(v' - E_v, 0)))
                                   1 sum                                         + u (5 c2 sqrt(v') + eps)
    q  = m' / d                    the division (2)                        E_q = 2 u |q| + (E_m + |q| E_d) / (d - E_d)
    s  = c1 q                      (float) c1 (1), 1 product               E_s = c1 (2 u |q| + E_q)
    p' = p - s                     its own rounding                        E_p = E_s + u |p'|

c1 = lr / (1 - b1^step) and c2 = 1 / sqrt(1 - b2^step) are formed in double (on the host with pow, in the kernel by
squaring) and converted to float: that conversion is the u charged above; the double arithmetic behind it (a relative
step * 2^-53 at most in b^step while b^step still matters) is covered by a relative 2^-40 on both.  sqrt is not
Lipschitz at 0, so the error of v' goes through the exact difference of square roots (downwards is the larger side of a
concave function), and the quotient's bound divides by the smallest denominator the kernel can have seen.
That is 22 roundings in all: 2 in g, 4 in m', 5 in v', 5 in d, 2 in q, 2 in s, 1 in p', and the 2^-40.  hipcc contracts
a product and the sum behind it into one FMA where it can; an FMA rounds once where the two operations round twice, so
the count above is an upper bound for either code.  The bound is first order in u; the neglected products of two
roundings are below 2^-20 of it, and every bound is multiplied by 1 + 2^-10.  Subnormal results are not modelled: the
tests keep every intermediate above 1e-30."""
import math

import torch

U = 2.0 ** -24
MASK64 = (1 << 64) - 1


def f32(x):
    """the float a hyper-parameter becomes when it crosses the C ABI, as a Python double"""
    return float(torch.tensor(x, dtype=torch.float32).item())


def adam_ref(p, g, m, v, step, lr, b1, b2, eps, wd, err=None):
    """One step of torch/optim/adam.py's _single_tensor_adam (L2 weight decay, no amsgrad / maximize) in float64 at the
    float32-rounded hyper-parameters -> ((p', m', v'), (E_p, E_m, E_v)): the three updated tensors and the elementwise
    rounding bound of adam_kernel's fp32 evaluation of each (module docstring).
    err = (E_p, E_m, E_v) of the step before, when the kernel's inputs are themselves its outputs (an iterated
    trajectory): they pass through the same derivatives (wd E_p into g, b1 E_m into m', b2 E_v into v', E_p into p'), so
    the bounds of a trajectory add up step by step."""
    lr, b1, b2, eps, wd = (f32(x) for x in (lr, b1, b2, eps, wd))
    p, g0, m0, v0 = (t.detach().double() for t in (p, g, m, v))
    step = int(step)
    c1 = lr / (1.0 - b1 ** step)
    c2 = 1.0 / math.sqrt(1.0 - b2 ** step)
    o1, o2 = 1.0 - b1, 1.0 - b2
    gg = g0 + wd * p
    m1 = b1 * m0 + o1 * gg
    v1 = b2 * v0 + o2 * gg * gg
    rv = v1.sqrt()
    d = rv * c2 + eps
    q = m1 / d
    p1 = p - c1 * q

    Ep0, Em0, Ev0 = err if err is not None else (0.0, 0.0, 0.0)
    G = g0.abs() + (wd * p).abs() + wd * Ep0
    E_g = U * (g0.abs() + 2.0 * (wd * p).abs()) + wd * Ep0
    E_m = U * (2.0 * (b1 * m0).abs() + 3.0 * o1 * G) + o1 * E_g + b1 * Em0
    E_v = U * (2.0 * b2 * v0.abs() + 4.0 * o2 * G * G) + 2.0 * o2 * G * E_g + b2 * Ev0
    E_d = c2 * (rv - (v1 - E_v).clamp_min(0.0).sqrt()) + U * (5.0 * c2 * rv + eps) + 2.0 ** -40 * c2 * rv
    d_lo = (d - E_d).clamp_min(1e-300)
    E_q = 2.0 * U * q.abs() + (E_m + q.abs() * E_d) / d_lo
    E_s = c1 * ((2.0 * U + 2.0 ** -40) * q.abs() + E_q)
    E_p = E_s + U * p1.abs() + Ep0
    slack = 1.0 + 2.0 ** -10
    return (p1, m1, v1), (E_p * slack, E_m * slack, E_v * slack)


def cross_entropy_ref(x, t, scale=None):
    """scale * sum over rows of (logsumexp(x[r]) - x[r, t[r]]) and its gradient (softmax - onehot) * scale in float64 from
    max / exp / log / sum alone, and the same two from stock fp32 torch on the CPU (the yardstick).  scale None: 1 / rows,
    torch.nn.CrossEntropyLoss()'s mean.  -> (loss64, grad64, loss32, grad32), the fp32 pair converted to float64."""
    x = x.detach().cpu()
    t = t.detach().cpu().long()
    rows = x.shape[0]
    x64 = x.double()
    mx = x64.max(dim=1, keepdim=True).values
    e = (x64 - mx).exp()
    s = e.sum(dim=1, keepdim=True)
    onehot = torch.zeros_like(x64)
    onehot[torch.arange(rows), t] = 1.0
    sc = 1.0 / rows if scale is None else float(scale)
    row_loss = s.log().squeeze(1) - (x64[torch.arange(rows), t] - mx.squeeze(1))
    loss64 = row_loss.sum().item() * sc
    grad64 = (e / s - onehot) * sc
    x32 = x.float().clone().requires_grad_(True)
    if scale is None:
        l32 = torch.nn.functional.cross_entropy(x32, t)
    else:
        l32 = torch.nn.functional.cross_entropy(x32, t, reduction="sum") * torch.tensor(sc, dtype=torch.float32)
    l32.backward()
    return loss64, grad64, float(l32.item()), x32.grad.double()


def ce_bounds(x, t, scale=None):
    """(loss64, grad64, loss bound, gradient bound): as close to fp64 as fp32 torch up to the factor 8 of
    test_gpu_grad_error.py, with the floor 2e-6 of test_gpu_optim.py"""
    l64, g64, l32, g32 = cross_entropy_ref(x, t, scale)
    lb = max(8.0 * abs(l32 - l64), 2e-6 * max(1.0, abs(l64)))
    gb = max(8.0 * (g32 - g64).abs().max().item(), 2e-6 * g64.abs().max().item())
    return l64, g64, lb, gb


def splitmix_advance(state):
    """what step_state_advance_kernel (pn_context.hip) and advance_step_state (pn_train.hip) do to {epoch, seed, adam_step}:
    epoch += 1, adam_step += 1, seed = splitmix64(seed), in Python integers"""
    z = (state["seed"] + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return {"epoch": state["epoch"] + 1, "seed": z ^ (z >> 31), "adam_step": state["adam_step"] + 1}


# ------------------------------------------------------------------------------------------------
# case tables of tests/test_gpu_loss_adam.py (held to the sources' constants by tests/test_optim_host.py)
# ------------------------------------------------------------------------------------------------
CE_ROWS = (1, 63, 64, 65, 1023, 1024, 1025, 32767, 32768, 32769, 65535, 65536, 65537)
CE_CLASSES = (1, 2, 63, 64, 65, 300)        # at 33 rows
CE_ONE_BLOCK_ROWS = 32768                   # up to here one workgroup stores the loss; beyond: memset + atomics
CE_SCALES = (3.0, 100.0, 1e3, 1e4)
ADAM_COUNTS = (1, 255, 256, 257, 2047, 2048, 2049, 4097)
ADAM_LIST_LENGTHS = (31, 32, 33, 64, 65)    # tensors of 17 elements
ADAM_STEPS = (1, 2, 10, 1000, 10 ** 6, 2 ** 31 - 1)
ADAM_HYPER = {                              # lr, (beta1, beta2), eps, weight decay
    "recipe": (0.005, (0.9, 0.999), 1e-8, 5e-4),
    "wd0": (0.005, (0.9, 0.999), 1e-8, 0.0),
    "eps1e-3": (0.005, (0.9, 0.999), 1e-3, 5e-4),
    "beta1_0": (0.005, (0.0, 0.999), 1e-8, 5e-4),
}
STATE_SEEDS = ((0, 0), (77, 3), (0x7FFFFFFFFFFFFFFF, 1000))      # (seed, first_epoch)


def ce_classes_for_rows(rows):
    return 2 if rows % 2 else 3


def adam_elements():
    """(p, g, m, v) fp32 [n]: the element classes of the single-step test, interleaved"""
    rows = []
    signs = (1.0, -1.0)
    k = 0
    for e in range(-12, 5):                 # |g| from 1e-12 to 1e4 by decades, warm state
        for mv in ((0.0, 0.0), (0.01, 1e-4)):
            rows.append((0.3 * signs[k % 2], 10.0 ** e * signs[(k // 2) % 2], mv[0] * signs[(k // 3) % 2], mv[1]))
            k += 1
    for p in (0.0, 1.0, -2.5):              # g == 0 with m == v == 0
        rows.append((p, 0.0, 0.0, 0.0))
    for p in (0.5, -0.5):                   # g == 0 with non-zero m, v
        rows.append((p, 0.0, 0.02, 3e-4))
        rows.append((p, 0.0, -1e-5, 1e-9))
    for e in range(-6, 4):                  # |p| from 1e-6 to 1e3
        rows.append((10.0 ** e * signs[e % 2], 0.01, 0.003, 2e-5))
        rows.append((10.0 ** e * signs[(e + 1) % 2], -1e-7, 0.0, 0.0))
    for vv in (1e-30, 1e-24, 1e-16):        # v tiny with m not
        rows.append((1.0, 1e-9, 0.1, vv))
        rows.append((-1.0, 0.0, -0.1, vv))
    t = torch.tensor(rows, dtype=torch.float32)
    return t[:, 0].contiguous(), t[:, 1].contiguous(), t[:, 2].contiguous(), t[:, 3].contiguous()
