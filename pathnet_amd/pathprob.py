"""Path likelihoods: how probable given paths are under a sampler's own tables (pn_path_prob, pn_prob.hip).

The walker's step -- ``slot = r0 % k``, ``next = r1 >= thr[slot] ? A : B`` with r0, r1 uniform on [0, 2^31) -- gives every
transition cur -> x the exact probability ``N(cur -> x) / 2^62``; the kernel returns the integers N (and, for the biased
walker, the table's mass per class and the class of the step taken), and the formulas below turn them into probabilities
in fp64.  The formulas are plain torch, so they run on CPU tensors as well.

``smp.path_prob(ids)`` -> PathProb under the plain table; ``smp.biased(p, q).path_prob(ids, kind="realised")`` under what
the biased walker does (at most 64 trials a step), ``kind="target"`` under the distribution it aims at.
``importance_weights(target, proposal)`` re-weights paths drawn from one walker to expectations under another.
"""
import collections
import ctypes
import math

import torch

from . import _lib

TWO62 = float(2 ** 62)
TWO32 = float(2 ** 32)
TRIALS = 64                 # PN_BIAS_MAX_TRIALS: trials 1..63 of a step may reject, the 64th is taken as it is
COUNTERS = ("bad_ids", "empty_tables", "impossible")


class PathProb(collections.namedtuple("PathProb", ("num", "step", "logp", "counters", "mass", "cls"))):
    """Tensors on the device of the ids; nothing has been read back.
    num int64 [..., W, L-1]       N(ids[t] -> ids[t+1]): the table's probability of the transition is num / 2^62
    step fp64 [..., W, L-1]       probability of every transition under the walker asked about
    logp fp64 [..., W]            sum over t of log(step), added in step order; -inf where a step is impossible
    counters int64 [4]            {ids outside [0, n) seen by a transition, transitions out of an empty table, impossible
                                  transitions (inside the graph, table not empty, N == 0), 0}
    mass int64 [..., W, L-1, 3]   biased only: the table's mass on class 0 (return) / 1 (near) / 2 (far) given ids[t-1]
    cls uint8 [..., W, L-1]       biased only: class of ids[t+1]; 3 = none (transition 0, or an id outside the graph)"""
    __slots__ = ()

    def summary(self):
        """A small dict of Python numbers (the one host read)."""
        fin = torch.isfinite(self.logp)
        flat = torch.cat((self.counters[:3].double(),
                          torch.stack((fin.sum().double(), torch.where(fin, self.logp, torch.zeros_like(self.logp)).sum()))))
        c0, c1, c2, possible, total = flat.cpu().tolist()
        out = dict(zip(COUNTERS, (int(c0), int(c1), int(c2))))
        out["paths"] = int(self.logp.numel())
        out["possible_paths"] = int(possible)
        out["mean_logp"] = total / possible if possible else None
        return out


def table_step(num):
    """num / 2^62 in fp64: the probability of every transition under the plain table."""
    return num.to(torch.float64) / TWO62


def path_logp(step):
    """log-likelihood of every path: the logs of its steps added in step order (fp64 [..., L-1] -> [...]); an impossible
    step makes it -inf.  A path of one node has no step and log-likelihood 0."""
    acc = torch.zeros(step.shape[:-1], dtype=torch.float64, device=step.device)
    for t in range(step.shape[-1]):
        acc = acc + torch.log(step[..., t])
    return acc


def _per_class(values, cls, device):
    """values (three Python floats) picked by class; class 3 picks 1.0"""
    return torch.tensor(list(values) + [1.0], dtype=torch.float64, device=device)[cls.long()]


def realised_step(num, mass, cls, thresholds):
    """What pn_sample_paths_biased does, exactly: a step proposes from the table, accepts a proposal of class c with
    probability a_c = T_c / 2^32 in each of its trials 1..63 and takes the 64th proposal as it is.  With alpha the chance
    that a trial accepts,
        P(x) = q_x a_cls (1 - (1 - alpha)^63) / alpha + (1 - alpha)^63 q_x,      q_x = num / 2^62,
    and P = q_x when alpha == 0.  1 - alpha is formed as beta = sum_c m_c (2^32 - T_c) / 2^32, without the subtraction, and
    its power through log1p / expm1, so a small alpha and a small beta both keep their digits.  A transition without a
    class (cls == 3: no prev) is the plain table step."""
    T = [float(int(t)) for t in thresholds]
    m = mass.to(torch.float64) / TWO62
    alpha = m[..., 0] * (T[0] / TWO32) + m[..., 1] * (T[1] / TWO32) + m[..., 2] * (T[2] / TWO32)
    beta = (m[..., 0] * ((TWO32 - T[0]) / TWO32) + m[..., 1] * ((TWO32 - T[1]) / TWO32) +
            m[..., 2] * ((TWO32 - T[2]) / TWO32))
    qx = table_step(num)
    a_cls = _per_class([t / TWO32 for t in T], cls, num.device)
    lb = torch.where(alpha < 0.5, torch.log1p(-alpha), torch.log(beta))
    safe = torch.where(alpha > 0, alpha, torch.ones_like(alpha))
    P = qx * a_cls * (-torch.expm1((TRIALS - 1) * lb)) / safe + torch.exp((TRIALS - 1) * lb) * qx
    return torch.where((alpha > 0) & (cls != 3), P, qx)


def target_step(num, mass, cls, p, q):
    """The distribution the biased walker aims at: P(x) = num w_cls / sum_c mass_c w_c with w = (1/p, 1, 1/q), 0 for an
    infinite parameter; 0 where the denominator is 0.  A transition without a class (cls == 3) is the plain table step."""
    w = [0.0 if math.isinf(p) else 1.0 / p, 1.0, 0.0 if math.isinf(q) else 1.0 / q]
    m = mass.to(torch.float64)
    den = m[..., 0] * w[0] + m[..., 1] * w[1] + m[..., 2] * w[2]
    safe = torch.where(den > 0, den, torch.ones_like(den))
    P = torch.where(den > 0, num.to(torch.float64) * _per_class(w, cls, num.device) / safe, torch.zeros_like(den))
    return torch.where(cls != 3, P, table_step(num))


def _launch(base, ids, second_order):
    """pn_path_prob over the tables of `base` -> num, mass, cls, counters (mass and cls None in first order)."""
    t = ids if isinstance(ids, torch.Tensor) else torch.as_tensor(ids)
    if t.dim() < 2:
        raise ValueError("path_prob: ids of shape [..., W, L] expected, got %s" % (tuple(t.shape),))
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise TypeError("path_prob: integer node ids expected, got %s" % t.dtype)
    if t.dtype != torch.int32:       # (a wider id cannot be a node: it stays out of range after the narrowing)
        t = t.clamp(-1, 2 ** 31 - 1).to(torch.int32)
    dev = base.device
    t = t.to(dev).contiguous()
    W, L = int(t.shape[-2]), int(t.shape[-1])
    if W < 1 or L < 1:
        raise ValueError("path_prob: paths of %d x %d nodes" % (W, L))
    rows = t.numel() // (W * L)
    lead = tuple(t.shape[:-1]) + (L - 1,)
    lib = _lib.load()
    tb = base._tables()
    need = ctypes.c_int64(0)
    _lib.check(lib.pn_path_prob_workspace_bytes(ctypes.byref(tb), W, L, rows, second_order, ctypes.byref(need)))
    with torch.cuda.device(dev):
        num = torch.empty(lead, dtype=torch.int64, device=dev)
        mass = torch.empty(lead + (3,), dtype=torch.int64, device=dev) if second_order else None
        cls = torch.empty(lead, dtype=torch.uint8, device=dev) if second_order else None
        counters = torch.empty(4, dtype=torch.int64, device=dev)         # the call zeroes it
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev) if need.value else None
        desc = _lib.PathProbOut(num.data_ptr(), mass.data_ptr() if second_order else None,
                                cls.data_ptr() if second_order else None, counters.data_ptr())
        _lib.check(lib.pn_path_prob(_lib.context(dev), ctypes.byref(tb), W, L, rows, _lib.ptr(t), second_order,
                                    ctypes.byref(desc), _lib.ptr(ws), need.value, _lib.stream_ptr(dev)))
    return num, mass, cls, counters


def path_prob(smp, ids):
    """Likelihood of the paths ids ``[..., W, L]`` (an int32 device tensor is read in place; anything else is narrowed and
    uploaded) under the plain walk of a MerwSampler / UniformSampler -> PathProb (mass and cls None).  Enqueued on the
    current stream; nothing is read back."""
    num, _, _, counters = _launch(smp, ids, 0)
    step = table_step(num)
    return PathProb(num, step, path_logp(step), counters, None, None)


def biased_path_prob(view, ids, kind="realised"):
    """Likelihood of the paths under the second-order walk of a BiasedSampler -> PathProb.  kind="realised": what the
    walker does, trial cap included (realised_step); kind="target": the distribution it aims at (target_step).
    Transition 0 is the plain table step either way.  The kernel call does not depend on (p, q)."""
    if kind not in ("realised", "target"):
        raise ValueError("path_prob: kind must be 'realised' or 'target', got %r" % (kind,))
    num, mass, cls, counters = _launch(view.base, ids, 1)
    if kind == "realised":
        step = realised_step(num, mass, cls, view.thresholds)
    else:
        step = target_step(num, mass, cls, view.p, view.q)
    return PathProb(num, step, path_logp(step), counters, mass, cls)


def importance_weights(target, proposal, normalize=True):
    """Weights that turn averages over paths drawn from `proposal` into expectations under `target` (two PathProb of the
    same ids): exp(target.logp - proposal.logp), fp64 ``[..., W]``.  A weight is 0 where the target is impossible (whatever
    the proposal says) and nan where only the proposal is: such a path cannot have been drawn from it.
    normalize: the weights of the W paths of a row are divided by their sum; a row whose weights sum to 0 stays 0."""
    if tuple(target.logp.shape) != tuple(proposal.logp.shape):
        raise ValueError("importance_weights: likelihoods of %s and of %s paths" % (tuple(target.logp.shape),
                                                                                    tuple(proposal.logp.shape)))
    tl, pl = target.logp, proposal.logp
    dead_t, dead_p = torch.isinf(tl) & (tl < 0), torch.isinf(pl) & (pl < 0)
    w = torch.exp(torch.where(dead_t | dead_p, torch.zeros_like(tl), tl - pl))
    w = torch.where(dead_p, torch.full_like(w, math.nan), w)
    w = torch.where(dead_t, torch.zeros_like(w), w)
    if normalize:
        s = w.sum(-1, keepdim=True)
        w = torch.where(s == 0, w, w / torch.where(s == 0, torch.ones_like(s), s))
    return w
