"""NumPy restatement of pn_ensemble_add / pn_ensemble_finish (include/pathnet_hip.h) and the error bounds its users hold
the kernels to.  Nothing here runs on a GPU.

The restatement works in a float type of the caller's choice: np.float64 is the definition the kernels implement,
np.longdouble (64-bit mantissa on x86) is the yardstick both are measured against.

Bounds.  u = 2^-53 is the unit roundoff of fp64: one correctly rounded operation has relative error <= u, and "k ulp" of a
library function is relative error <= 2 k u.  The ROCm device-library documentation is not shipped with the toolchain this
was written against, so exp and log are taken at 2 ulp each (E = L = 4 u); OpenCL's full-profile table, which the device
library follows, allows 3 ulp for both, and the measured error of either is below 1 ulp.

One sample, one row, C classes, x the fp32 logits (exact in fp64), m their maximum:
  d_c = x_c - m        one rounding, |error| <= u |d_c|.  exp(d) is exactly 0 below d = -746, so only |d_c| <= 746 matters
                       and the error of d moves exp(d) by a relative 746 u at the most.
  e_c = exp(d_c)       relative E on top:                                    (746 + E) u
  Z = sum_c e_c        C - 1 additions of non-negative terms, each term
                       already off by (746 + E) u:                           (C - 1 + 746 + E) u
  p_c = e_c / Z        the two above and one rounding:                       (C + 2 (746 + E)) u
                       REL_P(C) = (C + 2 (E + 746) + 4) u leaves room for the second-order terms.
  An e_c in the subnormal range (d_c < -708) has an absolute, not a relative, error: at most 2^-1074 each, far below
  TINY = 1e-300, which every bound carries as an absolute floor.
K samples: psum = sum_k p adds K - 1 roundings of a growing non-negative sum:
  |psum - exact| <= (REL_P + K u) psum + TINY.
Entropy of one sample, h = -sum_c p_c log p_c.  A relative error r_c of p_c moves p_c log p_c by |(log p_c + 1) p_c r_c|
<= (|p_c log p_c| + p_c) REL_P; log adds L u |p_c log p_c|, the product one rounding, the C-term sum (C - 1) u sum |p log p|.
With sum_c p_c = 1 and sum_c |p_c log p_c| = h:
  |h - exact| <= REL_P (1 + h) + (C + L) u h.
Over K samples, plus the K - 1 additions:  |hsum - exact| <= REL_P (K + hsum) + (C + L + K) u hsum + TINY.
The mean distribution q = psum / n carries psum's relative error and one rounding, so its entropy obeys the single-sample
formula with REL_Q = REL_P + (K + 1) u in place of REL_P.

fp32 outputs: the fp64 value rounded once.  Where the fp64 error is a relative one far below 2^-24 (prob, confidence,
agreement) two implementations differ by at most ONE fp32 ulp, when their fp64 values straddle a rounding boundary.
entropy and mutual_info are different: their fp64 error is ABSOLUTE (REL_P (1 + h): a row that is sure of itself has
h ~ 1e-12 and an error of 1e-16 all the same, and mutual_info is a difference of two nearly equal numbers), so for them the
fp64 bound of the expression is added to the one ulp.
"""
import collections

import numpy as np

U = 2.0 ** -53
E_EXP = 4.0         # 2 ulp, in units of u
L_LOG = 4.0         # 2 ulp
TINY = 1e-300
MAX_CLASSES = 4096
ROUTE_NONE, ROUTE_THREAD, ROUTE_WAVE, ROUTE_BLOCK = 0, 1, 2, 3

State = collections.namedtuple("State", ("psum", "hsum", "votes", "count", "bad"))
Result = collections.namedtuple("Result", ("prob", "label", "vote_label", "confidence", "entropy", "mutual_info", "agreement",
                                           "confusion", "skipped", "exact"))


def rel_p(C):
    return (C + 2.0 * (E_EXP + 746.0) + 4.0) * U


def tol_psum(psum, C, K):
    """absolute bound of every entry of psum after K samples"""
    return (rel_p(C) + K * U) * np.asarray(psum, np.float64) + TINY


def tol_entropy(h, C, rel):
    return rel * (1.0 + np.asarray(h, np.float64)) + (C + L_LOG) * U * np.asarray(h, np.float64) + TINY


def tol_hsum(hsum, count, C, K):
    hsum = np.asarray(hsum, np.float64)
    return rel_p(C) * (np.asarray(count, np.float64) + hsum) + (C + L_LOG + K) * U * hsum + TINY


def new_state(rows, C, dtype=np.float64):
    return State(np.zeros((rows, C), dtype), np.zeros(rows, dtype), np.zeros((rows, C), np.int32),
                 np.zeros(rows, np.int32), np.zeros(rows, np.int32))


def _plogp(p):
    out = np.zeros_like(p)
    pos = p > 0
    out[pos] = p[pos] * np.log(p[pos])
    return out


def add(state, logits, index=None):
    """pn_ensemble_add: logits fp32 [R, S, C] (or [S, C]) into `state`, in place -> status (logits rows skipped)"""
    x = np.asarray(logits, np.float32)
    if x.ndim == 2:
        x = x[None]
    R, S, C = x.shape
    rows = state.count.shape[0]
    dt = state.psum.dtype
    row = np.arange(S, dtype=np.int64) if index is None else np.asarray(index, np.int64)
    ok = (row >= 0) & (row < rows)
    status = int(R * (~ok).sum())
    src, dst = np.flatnonzero(ok), row[ok]
    assert len(set(dst.tolist())) == len(dst), "duplicate index entries in one call"
    for r in range(R):
        xr = x[r, src]
        fin = np.isfinite(xr).all(axis=1)
        state.bad[dst[~fin]] += 1
        xs, d = xr[fin], dst[fin]
        if not len(d):
            continue
        m = xs.max(axis=1, keepdims=True)
        e = np.exp(xs.astype(dt) - m.astype(dt))
        p = e / e.sum(axis=1, keepdims=True)
        state.psum[d] += p
        state.hsum[d] += -_plogp(p).sum(axis=1)
        state.votes[d, xs.argmax(axis=1)] += 1          # (numpy's argmax: the first of equal entries)
        state.count[d] += 1
    return status


def finish(state, subset=None, target=None):
    """pn_ensemble_finish -> Result.  The float members are fp32, rounded once from the state's float type; `exact` holds
    (entropy, mean sample entropy) before rounding, for the bounds."""
    rows, C = state.psum.shape
    row = np.arange(rows, dtype=np.int64) if subset is None else np.asarray(subset, np.int64)
    inside = (row >= 0) & (row < rows)
    safe = np.where(inside, row, 0)
    cnt = np.where(inside, state.count[safe] if rows else 0, 0).astype(np.int64)
    live = cnt > 0
    n = np.where(live, cnt, 1).astype(state.psum.dtype)
    psum = np.where(live[:, None], state.psum[safe] if rows else 0, 0)
    votes = np.where(live[:, None], state.votes[safe] if rows else 0, 0)
    q = psum / n[:, None]
    label = np.where(live, psum.argmax(axis=1) if C else 0, -1).astype(np.int64)
    vote_label = np.where(live, votes.argmax(axis=1) if C else 0, -1).astype(np.int64)
    ent = -_plogp(q).sum(axis=1)
    hbar = np.where(live, (state.hsum[safe] if rows else 0), 0) / n
    at = np.where(live, label, 0)
    pick = np.arange(len(row))
    conf = np.where(live, psum[pick, at] / n, 0)
    agree = np.where(live, votes[pick, at].astype(state.psum.dtype) / n, 0)
    mi = np.maximum(0, ent - hbar)
    confusion = skipped = None
    if target is not None:
        t = np.where(inside, np.asarray(target, np.int64)[safe] if rows else 0, 0)
        t_ok = (t >= 0) & (t < C)
        confusion = np.zeros((C, C), np.int64)
        use = inside & t_ok & (label >= 0)
        np.add.at(confusion, (t[use], label[use]), 1)
        skipped = np.array([(inside & ~t_ok).sum(), (label < 0).sum()], np.int64)
    f32 = lambda a: np.asarray(a).astype(np.float32)         # noqa: E731
    return Result(f32(q), label, vote_label, f32(conf), f32(ent), f32(mi), f32(agree), confusion, skipped,
                  (np.asarray(ent, np.float64), np.asarray(hbar, np.float64)))


def route(rows, C):
    """the documented work split (include/pathnet_hip.h), for the comparison with pn_ensemble_route"""
    if rows == 0:
        return ROUTE_NONE
    return ROUTE_THREAD if C <= 16 else ROUTE_WAVE if C <= 1024 else ROUTE_BLOCK


def ulp32(a):
    return np.spacing(np.abs(np.asarray(a, np.float32)))


# ---- the case table of tests/test_gpu_ensemble.py: (C, S, R) -- the larger C with the smaller S -------------------------------
C_VALUES = (1, 2, 7, 63, 64, 65, 257, 4096)
S_VALUES = (0, 1, 63, 64, 65, 1000)
R_VALUES = (1, 2, 5)
BOUNDARY_C = (16, 17, 1024, 1025)          # both sides of every boundary pn_ensemble_route has in C


def case_table():
    cases = []
    s_desc = sorted(S_VALUES, reverse=True)
    for i, C in enumerate(C_VALUES):
        # every C meets S = 0 and S = 1; the larger sizes go round, shifted so that a larger C gets a smaller S
        sizes = {0, 1, s_desc[min(i, len(s_desc) - 3)], s_desc[min(i + 1, len(s_desc) - 3)]}
        if C <= 64:
            sizes |= {63, 64, 65}
        for S in sorted(sizes):
            for R in R_VALUES:
                if S * C * R <= 400_000:
                    cases.append((C, S, R))
    for C in BOUNDARY_C:
        for S, R in ((1, 2), (5, 1), (65, 2)):
            cases.append((C, S, R))
    cases.append((4096, 5, 2))
    cases.append((7, 1000, 5))
    return sorted(set(cases))


def make_logits(kind, R, S, C, seed):
    """the input families of the issue -> fp32 [R, S, C]"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((R, S, C)) * 3).astype(np.float32)
    if kind == "normal":
        return x
    if kind == "large":         # magnitude 1e4; every third row spreads over more than 746
        x = (x + np.float32(1e4) * rng.choice([-1.0, 1.0], size=(R, S, 1))).astype(np.float32)
        if C > 1:
            x[:, ::3, 0] -= np.float32(800.0)
            x[:, 1::3, C - 1] += np.float32(2000.0)
        return x
    if kind == "nonfinite":     # rows 0 mod 4: one bad value in sample 0 only; rows 1 mod 4: bad in every sample
        vals = (np.nan, np.inf, -np.inf)
        for s in range(S):
            if s % 4 == 0:
                x[0, s, (s // 4) % C] = vals[(s // 4) % 3]
            elif s % 4 == 1:
                x[:, s, (s // 4) % C] = vals[(s // 4) % 3]
        return x
    if kind == "ties":          # bit-identical columns: the top value sits in two (three) columns of every row
        if C > 1:
            top = np.abs(x).max(axis=2) + np.float32(1.0)
            hi = rng.integers(1, C, size=S)
            lo = (hi * rng.random(S)).astype(np.int64)         # lo < hi
            for s in range(S):
                x[:, s, hi[s]] = top[:, s]
                x[:, s, lo[s]] = top[:, s]
                if C > 2:
                    x[:, s, (hi[s] + lo[s]) // 2] = top[:, s]
        return x
    if kind == "margin":        # one class ahead by far more than any bound: every discrete output is decidable
        lead = rng.integers(0, C, size=S)
        for s in range(S):
            x[:, s, lead[s]] = np.abs(x[:, s]).max() + np.float32(4.0)
        return x
    raise ValueError(kind)


KINDS = ("normal", "large", "nonfinite", "ties", "margin")
