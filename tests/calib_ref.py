"""NumPy restatement of pn_calib_sweep, pn_ensemble_add_scaled and pn_calib_stats (include/pathnet_hip.h) and the error
bounds their users hold the kernels to.  Nothing here runs on a GPU.

As in ensemble_ref.py the restatement works in a float type of the caller's choice: np.float64 is the definition the kernels
implement, np.longdouble the yardstick both are measured against.  u, E (exp) and L (log) are ensemble_ref's.

Bounds, relative to ensemble_ref's derivation of REL_P:
  a_c = (x_c - m) * inv     three roundings (the difference, inv = 1 / tau, the product) where the plain softmax has one, so
                            |a_c|'s relative error is 3 u; exp(a) is exactly 0 below a = -746, so only |a_c| <= 746 matters
                            and the error of a moves exp(a) by a relative 3 * 746 u at the most.
  e_c, Z, p_c               as in ensemble_ref with 3 * 746 in place of 746:
                            REL_PS(C) = (C + 2 (E + 3 * 746) + 4) u.
  Scaled add: psum, hsum and the entropy obey ensemble_ref's formulas with REL_PS in place of REL_P.
  q = (sum_r p_y) / n_ok    R - 1 additions of a growing non-negative sum and one division:  REL_Q = REL_PS + (R + 1) u.
  row_nll = -log q          log turns q's relative error into an absolute one, and adds L u |log q| of its own:
                            |row_nll - exact| <= REL_Q + L u |log q| + TINY.
                            (An e_y in the subnormal range has an absolute error of 2^-1074 instead; that only matters for a q
                            that is itself near the bottom of the range, which no case here holds.)
  nll[t] = sum_s row_nll    S - 1 additions in whatever order: (S - 1) u sum_s |row_nll| on top of the rows' own bounds.
Statistics (inputs are fp32, exact in fp64):
  -log p                    L u |log p| per row; the sum over n rows adds (n - 1) u sum |term|:   (n + L) u sum |term| + TINY
  Brier                     a row is C terms (d = p - [c == y]: one rounding, d d: one, C - 1 additions, or fewer roundings with
                            a fused multiply-add), the rows' sum n - 1 more, all terms non-negative:  (n + C + 3) u sum + TINY
  aurc                      err / k: one rounding, m - 1 additions, one division:                    (m + 2) u aurc + TINY
Everything else -- bins, counts, order, err_prefix, best, tau -- is integer or a copied grid member: exact.
"""
import collections

import numpy as np

import ensemble_ref as eref

U, E_EXP, L_LOG, TINY = eref.U, eref.E_EXP, eref.L_LOG, eref.TINY
PART = 256              # rows per partial of a column sum

Sweep = collections.namedtuple("Sweep", ("row_nll", "nll", "best", "tau", "counts", "q"))
Stats = collections.namedtuple("Stats", ("bin_count", "bin_correct", "bin_conf", "counts", "sums", "order", "err_prefix",
                                         "aurc", "used"))


def rel_ps(C):
    return (C + 2.0 * (E_EXP + 3 * 746.0) + 4.0) * U


def tol_row_nll(q, C, R):
    """absolute bound of row_nll, given the row's mean target probability q (0 where the row is unused)"""
    q = np.asarray(q, np.float64)
    logq = np.abs(np.log(np.where(q > 0, q, 1.0)))
    return rel_ps(C) + (R + 1) * U + L_LOG * U * logq + TINY


def tol_nll(row_nll, tol_rows):
    """absolute bound of every column sum"""
    S = row_nll.shape[0]
    return tol_rows.sum(axis=0) + max(S - 1, 0) * U * np.abs(np.asarray(row_nll, np.float64)).sum(axis=0) + TINY


def tol_psum_scaled(psum, C, K):
    return (rel_ps(C) + K * U) * np.asarray(psum, np.float64) + TINY


def tol_hsum_scaled(hsum, count, C, K):
    hsum = np.asarray(hsum, np.float64)
    return rel_ps(C) * (np.asarray(count, np.float64) + hsum) + (C + L_LOG + K) * U * hsum + TINY


def tol_stats_nll(total, n):
    return (n + L_LOG) * U * abs(float(total)) + TINY


def tol_stats_brier(total, n, C):
    return (n + C + 3) * U * abs(float(total)) + TINY


def tol_aurc(aurc, m):
    return (m + 2) * U * abs(float(aurc)) + TINY


def _finite_positive(t):
    return np.isfinite(t) & (t > 0)


def column_sums(row_nll):
    """partials of PART rows added in ascending s, the partials in ascending order (the documented order)"""
    S, T = row_nll.shape
    total = np.zeros(T, row_nll.dtype)
    for s0 in range(0, S, PART):
        part = np.zeros(T, row_nll.dtype)
        for s in range(s0, min(s0 + PART, S)):
            part = part + row_nll[s]
        total = total + part
    return total


def sweep(logits, target, temps, dtype=np.float64):
    """pn_calib_sweep -> Sweep (best and tau are Python numbers; q [S, T] is the mean target probability, for the bounds)"""
    x = np.asarray(logits, np.float32)
    R, S, C = x.shape
    y = np.asarray(target, np.int64)
    temps = np.asarray(temps, np.float64)
    T = len(temps)
    t_ok = _finite_positive(temps)
    y_ok = (y >= 0) & (y < C)
    ys = np.where(y_ok, y, 0)
    acc = np.zeros((S, T), dtype)
    n_ok = np.zeros(S, np.int64)
    with np.errstate(all="ignore"):
        inv = np.where(t_ok, dtype(1) / np.where(t_ok, temps, 1.0).astype(dtype), dtype(1))
        for r in range(R):
            fin = np.isfinite(x[r]).all(axis=1) & y_ok
            idx = np.flatnonzero(fin)
            if not len(idx):
                continue
            xs = x[r, idx]
            d = xs.astype(dtype) - xs.max(axis=1, keepdims=True).astype(dtype)
            dy = d[np.arange(len(idx)), ys[idx]]
            for t in range(T):
                z = np.exp(d * inv[t]).sum(axis=1)
                acc[idx, t] += np.exp(dy * inv[t]) / z
            n_ok[idx] += 1
        used = y_ok & (n_ok > 0)
        q = np.where(used[:, None] & t_ok[None, :], acc / np.maximum(n_ok, 1)[:, None].astype(dtype), 0)
        row_nll = np.where(q > 0, -np.log(np.where(q > 0, q, 1)), np.where(used[:, None] & t_ok[None, :], np.inf, 0))
        row_nll = row_nll.astype(dtype)
        nll = column_sums(row_nll)
    nll = np.where(t_ok, nll, np.inf) if S else np.zeros(T, dtype)      # (S == 0 launches nothing: no grid entry is looked at)
    counts = np.array([used.sum(), (~y_ok).sum(), (y_ok & (n_ok == 0)).sum()], np.int64)
    best = -1
    if counts[0] > 0:
        for t in range(T):
            if np.isfinite(nll[t]) and (best < 0 or nll[t] < nll[best]):
                best = t
    tau = float(temps[best]) if best >= 0 else 1.0
    return Sweep(row_nll, nll, best, tau, counts, np.asarray(q, np.float64))


def add_scaled(state, logits, tau, index=None):
    """pn_ensemble_add_scaled: as ensemble_ref.add with exp((x - m) / tau) -> status"""
    x = np.asarray(logits, np.float32)
    if x.ndim == 2:
        x = x[None]
    R, S, C = x.shape
    if not (np.isfinite(tau) and tau > 0):
        return R * S
    rows = state.count.shape[0]
    dt = state.psum.dtype
    inv = dt.type(1) / dt.type(tau)
    row = np.arange(S, dtype=np.int64) if index is None else np.asarray(index, np.int64)
    ok = (row >= 0) & (row < rows)
    src, dst = np.flatnonzero(ok), row[ok]
    for r in range(R):
        xr = x[r, src]
        fin = np.isfinite(xr).all(axis=1)
        state.bad[dst[~fin]] += 1
        xs, d = xr[fin], dst[fin]
        if not len(d):
            continue
        m = xs.max(axis=1, keepdims=True)
        e = np.exp((xs.astype(dt) - m.astype(dt)) * inv)
        p = e / e.sum(axis=1, keepdims=True)
        state.psum[d] += p
        state.hsum[d] += -eref._plogp(p).sum(axis=1)
        state.votes[d, xs.argmax(axis=1)] += 1
        state.count[d] += 1
    return int(R * (~ok).sum())


def stats(conf, label, target, prob, C, B, dtype=np.float64):
    """pn_calib_stats from zeroed accumulators -> Stats (sums None without prob)"""
    conf = np.asarray(conf, np.float32)
    label, target = np.asarray(label, np.int64), np.asarray(target, np.int64)
    n = len(conf)
    with np.errstate(invalid="ignore"):
        no_label = label < 0
        bad_target = ~no_label & ((target < 0) | (target >= C))
        bad_conf = ~no_label & ~bad_target & ~((conf >= 0) & (conf <= 1))
    used = ~(no_label | bad_target | bad_conf)
    cd = conf.astype(np.float64)
    bin_count, bin_correct, bin_conf = (np.zeros(B, np.int64) for _ in range(3))
    b = np.minimum(B - 1, np.floor(np.where(used, cd, 0) * B).astype(np.int64))
    np.add.at(bin_count, b[used], 1)
    np.add.at(bin_correct, b[used], (label == target)[used].astype(np.int64))
    np.add.at(bin_conf, b[used], np.rint(cd[used] * 2.0 ** 32).astype(np.int64))
    zero_prob = 0
    sums = None
    if prob is not None:
        p = np.asarray(prob, np.float32).reshape(n, C)
        i = np.flatnonzero(used)
        py = p[i, target[i]].astype(dtype)
        zero_prob = int((py <= 0).sum())
        onehot = np.zeros((len(i), C), dtype)
        onehot[np.arange(len(i)), target[i]] = 1
        sums = np.array([(-np.log(py[py > 0])).sum(), ((p[i].astype(dtype) - onehot) ** 2).sum()], dtype)
    counts = np.array([used.sum(), no_label.sum(), bad_target.sum(), bad_conf.sum(), zero_prob], np.int64)
    bits = np.where(conf == 0, 0, conf.view(np.int32)).astype(np.int64)
    key = np.where(used, 0x3F800000 - bits, 2 ** 31 - 1)
    order = np.argsort(key, kind="stable").astype(np.int32)
    err = (used & (label != target)).astype(np.int64)
    err_prefix = np.cumsum(err[order]).astype(np.int32)
    m = int(used.sum())
    aurc = dtype(0)
    if m:
        aurc = (err_prefix[:m].astype(dtype) / np.arange(1, m + 1).astype(dtype)).sum() / dtype(m)
    return Stats(bin_count, bin_correct, bin_conf, counts, sums, order, err_prefix, aurc, used)


def ece_mce(bin_count, bin_correct, bin_conf):
    """expected and maximum calibration error from the exact bin integers"""
    cnt = np.asarray(bin_count, np.float64)
    m = cnt.sum()
    if m == 0:
        return 0.0, 0.0
    live = cnt > 0
    gap = np.zeros(len(cnt))
    gap[live] = np.abs(np.asarray(bin_correct, np.float64)[live] / cnt[live]
                       - np.asarray(bin_conf, np.float64)[live] / 2.0 ** 32 / cnt[live])
    return float((cnt / m * gap).sum()), float(gap.max())


# ---- the sweep's input family and case table ---------------------------------------------------------------------------------
DEFAULT_GRID = 2.0 ** (np.arange(-12, 13) / 4.0)
TRUE_TEMPS = (0.5, 1.0, 3.0)


def grid_of(T):
    if T == 25:
        return DEFAULT_GRID.copy()
    if T == 1:
        return np.array([1.0])
    if T == 2:
        return np.array([0.5, 2.0])
    if T == 3:
        return np.array([0.5, 1.0, 2.0])
    return 2.0 ** np.linspace(-3.0, 3.0, T)


def make_case(C, S, R, true, seed):
    """base ~ N(0, 4) [S, C]; logits = true (base + 0.3 noise[R, S, C]) in fp32; labels drawn from softmax(base) for S >= 64
    and argmin(base) below (a tiny, correctly labelled set underflows to nll == 0 at several grid points) -> logits, labels"""
    rng = np.random.default_rng(seed)
    base = 2.0 * rng.standard_normal((S, C))
    x = (true * (base[None] + 0.3 * rng.standard_normal((R, S, C)))).astype(np.float32)
    if S >= 64:
        p = np.exp(base - base.max(axis=1, keepdims=True))
        cdf = np.cumsum(p / p.sum(axis=1, keepdims=True), axis=1)
        y = np.minimum((rng.random((S, 1)) > cdf).sum(axis=1), C - 1)
    else:
        y = base.argmin(axis=1) if S else np.zeros(0, np.int64)
    return x, y.astype(np.int64)


# (C, S, R, T): every C, S, R and T of the issue; the larger C with the smaller S (ensemble_ref's S C R <= 400 000), and
# S C R T small enough for the long-double restatement.  255 / 256 / 257: both sides of the column sum's partial size.
SWEEP_CASES = (
    (1, 5, 2, 3), (1, 64, 1, 25), (2, 1, 1, 1), (2, 65, 2, 2), (2, 1000, 5, 25), (7, 0, 2, 25), (7, 63, 5, 256), (7, 255, 1, 3),
    (7, 256, 2, 25), (7, 257, 5, 2), (7, 1000, 2, 25), (7, 1000, 1, 256), (16, 64, 2, 25), (17, 65, 1, 25), (17, 1, 5, 3),
    (64, 257, 2, 25), (65, 63, 5, 25), (1024, 5, 2, 25), (1024, 65, 1, 3), (1025, 5, 2, 25), (1025, 64, 1, 2),
    (4096, 0, 1, 1), (4096, 1, 5, 25), (4096, 5, 2, 3),
)
SWEEP_KINDS = ("base", "nonfinite", "badtarget", "badgrid")


def sweep_inputs(kind, case):
    """-> logits [R, S, C], target [S], temps [T] of one family of one case"""
    C, S, R, T = case
    i = SWEEP_CASES.index(case)
    x, y = make_case(C, S, R, TRUE_TEMPS[i % 3], seed=100 + i)
    temps = grid_of(T)
    if kind == "nonfinite":     # rows 0 mod 4: one bad value in sample 0 only; rows 1 mod 4: bad in every sample
        vals = (np.nan, np.inf, -np.inf)
        for s in range(S):
            if s % 4 == 0:
                x[0, s, (s // 4) % C] = vals[(s // 4) % 3]
            elif s % 4 == 1:
                x[:, s, (s // 4) % C] = vals[(s // 4) % 3]
    elif kind == "badtarget":
        y[::5] = -1
        y[2::5] = C
        y[3::25] = 2 ** 40
    elif kind == "badgrid":
        bad = (0.0, -1.0, np.inf, np.nan, -np.inf)
        for j in range(0, T, 4):
            temps[j] = bad[(j // 4) % len(bad)]
    elif kind != "base":
        raise ValueError(kind)
    return x, y, temps


def sweep_cases(kind):
    """the non-base families run where the long-double restatement is cheap"""
    return [c for c in SWEEP_CASES if kind == "base" or c[0] * c[1] * c[2] * c[3] <= 1_000_000]


def decidable(lo, hi, C, R):
    """`best` does not hang on a rounding: the gap between the lowest and the second-lowest finite nll is at least 1000 x the
    sum of their bounds, or the two are bit-equal in both float types (the C = 1 tie, which the lowest t wins) -> (bool, gap
    in units of the bound)"""
    fin = np.flatnonzero(np.isfinite(lo.nll))
    if len(fin) < 2 or lo.counts[0] == 0:
        return True, np.inf
    tol = tol_nll(hi.row_nll.astype(np.float64), tol_row_nll(hi.q, C, R))
    a, b = fin[np.argsort(lo.nll[fin], kind="stable")[:2]]
    if lo.nll[a] == lo.nll[b] and hi.nll[a] == hi.nll[b]:
        return True, np.inf
    ratio = float((lo.nll[b] - lo.nll[a]) / (tol[a] + tol[b]))
    return ratio >= 1000.0, ratio


# ---- the statistics' case table -------------------------------------------------------------------------------------------------
STATS_N = (0, 1, 63, 64, 65, 255, 256, 257, 1000)
STATS_B = (1, 2, 15, 16, 1024)


def stats_inputs(n, C, seed):
    """confidences on the bin edges k / 16, exactly 0.0 and 1.0, repeated values; rows with label -1, a target out of range,
    a refused confidence and prob[target] == 0 -> conf, label, target, prob (prob's argmax is not tied to conf: the kernel
    takes them as given)"""
    rng = np.random.default_rng(seed)
    prob = rng.random((n, C)).astype(np.float32)
    prob /= np.maximum(prob.sum(axis=1, keepdims=True), np.float32(1e-30))
    pool = np.concatenate([np.arange(17) / 16.0, rng.random(24)]).astype(np.float32)      # edges, 0.0, 1.0, some others
    conf = pool[rng.integers(0, len(pool), size=n)]
    label = rng.integers(0, C, size=n).astype(np.int64)
    target = np.where(rng.random(n) < 0.6, label, rng.integers(0, C, size=n)).astype(np.int64)
    for k, (arr, val) in enumerate(((label, -1), (target, -1), (target, C), (conf, np.nan), (conf, 1.5), (conf, -0.25))):
        arr[7 + k::23] = val
    rows = np.arange(11, n, 19)
    rows = rows[(target[rows] >= 0) & (target[rows] < C)]
    prob[rows, target[rows]] = 0.0
    if n > 40:
        conf[30], conf[31] = np.float32(-0.0), np.float32(1.0)
    return conf, label, target, prob
