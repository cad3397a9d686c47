"""NumPy restatement of pn_explain_groups / pn_explain_totals (include/pathnet_hip.h) and the error bounds its users hold the
kernels to.  Nothing here runs on a GPU.

The restatement works in a float type of the caller's choice: np.float64 is the definition the kernels implement,
np.longdouble (64-bit mantissa on x86) is the yardstick both are measured against.

Bounds.  u = 2^-53; one correctly rounded operation has relative error <= u.  exp and log are taken at 2 ulp (E = L = 4 u), as
in ensemble_ref.py.  Inputs are fp32, exact in fp64, and a product of two of them is exact in fp64 (48 bits).

  t_j[c] = sum_h w[c,H+h] state[j,h]   exact products, H - 1 additions:  |err| <= H u A_t,   A_t = sum_h |w| |state|
  contribution = coef t / W            two more roundings:               |err| <= (H + 2) u A_con,  A_con = |coef| A_t / W
  e[c] = b + sum_h w[c,h] ego[h]       H additions:                      |err| <= (H + 1) u A_e,    A_e = |b| + sum_h |w| |ego|
  a sum over a set M of <= W members   the terms' errors and W - 1 additions:  |err| <= (H + W + 2) u A_M,  A_M = sum_M A_con
  Om, Om_R, Om_rest, K, K_R, K_rest    sums of <= W non-negative terms (the weights are positive; with renorm the coefficients
                                       are softmax weights, >= 0 -- the bound ASSUMES that): relative (W - 1) u each
  rho = (Om / Om_x) (K / K_x)          four sums, two divisions, one product:   relative (4 W + 3) u
  x = e + rho sum_M (one fma)          |err| <= u [(H + 5 W + 6) |rho| A_M + (H + 2) A_e]  =: tol_logits
                                       (|x| <= |rho| A_M + A_e covers the fma's own rounding)
  lse(x) = m + log sum_c exp(x_c - m)  x_c - m rounds once and matters only above -746, so exp's argument moves it by a
                                       relative 746 u at most, exp adds E u.  The kernel keeps a running (max, sum) per lane and
                                       merges lanes and class chunks, each merge rescaling a partial sum by one more exp of a
                                       rounded difference: (746 + E + 2) u per rescaling, and a term sees fewer than 2 C + 6 of
                                       them (<= C new maxima in its lane, one per lane to the common maximum -- 6 are allowed
                                       for, one per butterfly step -- and <= C chunks); the restatement's
                                       two-pass form sees none.  With the C + 6 additions of non-negative terms the sum is off by
                                       a relative [(2 C + 7)(746 + E + 2) + C + 6] u, which is the ABSOLUTE error of its log
                                       (the sum is >= 1, its log in [0, log C]); log itself adds L u log C and the final
                                       addition u |lse|:   LSE_ABS(C) + u |lse|
                                       A perturbation d of every x_c moves lse by at most d.
  lp(x) = x_t - lse(x)                 |err| <= 2 max_c tol_logits + LSE_ABS(C) + u (|lse| + |lp|)  =: tol_lp
  drop_delta, keep_gain                differences of two lp:  tol_lp + tol_lp + u |difference|

These are absolute bounds: drop_delta of a group that hardly matters is a difference of two nearly equal numbers.  An fp32
output is the fp64 value rounded once, so it is held to ONE fp32 ulp of the rounded reference plus the bound above.

pn_explain_totals: a running sum of n fp32 values (exact in fp64) is off by at most (n - 1) u sum |v|; the integers are exact.
"""
import collections

import numpy as np

U = 2.0 ** -53
E_EXP = 4.0
L_LOG = 4.0
TINY = 1e-300
NORM_SUM, NORM_COUNT = 0, 1
ROUTE_NONE, ROUTE_ROW, ROUTE_CHUNKED = 0, 1, 2
MAX_CON, TILE_FLOATS = 4096, 7168

FIELDS = ("full", "contribution", "drop_logits", "keep_logits", "drop_delta", "keep_gain", "flip", "present", "target_used",
          "status", "e", "rho_d", "rho_k", "tol")
Result = collections.namedtuple("Result", FIELDS)
Totals = collections.namedtuple("Totals", ("rows_present", "members", "flips", "drop_delta_sum", "keep_gain_sum"))


def ulp32(a):
    return np.spacing(np.abs(np.asarray(a, np.float32))).astype(np.float64)


def lse_abs(C):
    return ((2 * C + 7) * (746.0 + E_EXP + 2) + C + 6 + L_LOG * np.log(max(C, 1))) * U


def _lse(x):
    m = x.max(axis=-1, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))[..., 0]


def _lp(x, t):
    """x [..., C], t scalar class -> (lp, lse)"""
    l = _lse(x)
    return x[..., t] - l, l


def live_of(weight, shape, fi=np.float32):
    if weight is None:
        return np.ones(shape, bool), np.ones(shape, fi)
    w = np.asarray(weight, fi)
    with np.errstate(invalid="ignore"):
        lv = np.isfinite(w) & (w > 0)
    return lv, np.where(lv, w, fi(0))


def groups(state, coef, ego, fc2_w, fc2_b, weight, group, G, norm, renorm, target=None, dtype=np.float64,
           in_dtype=np.float32):
    """pn_explain_groups.  state fp32 [S, W, H], coef [S, W], ego [S, H], fc2_w [C, 2H], fc2_b [C], weight [S, W] or None,
    group int [S, W], target int [S] or None -> Result.  The float members are in `dtype` (round them with f32()); `tol` holds
    the fp64 bounds of the docstring, per output name, as float64 arrays.  in_dtype: what the inputs are read as (the kernels
    read fp32; the host tests feed an fp64 reference's own values)."""
    dt, fi = dtype, in_dtype
    state, coef, ego = np.asarray(state, fi), np.asarray(coef, fi), np.asarray(ego, fi)
    fc2_w, fc2_b, group = np.asarray(fc2_w, fi), np.asarray(fc2_b, fi), np.asarray(group, np.int64)
    S, W, H = state.shape
    C = fc2_w.shape[0]
    we, wp = fc2_w[:, :H].astype(dt), fc2_w[:, H:2 * H].astype(dt)
    live, wv = live_of(weight, (S, W), fi)
    full = np.zeros((S, C), dt)
    con = np.zeros((S, W, C), dt)
    e_all = np.zeros((S, C), dt)
    dl, kl = np.zeros((S, G, C), dt), np.zeros((S, G, C), dt)
    dd, kg = np.zeros((S, G), dt), np.zeros((S, G), dt)
    rho_d, rho_k = np.zeros((S, G), np.float64), np.zeros((S, G), np.float64)
    flip, present = np.zeros((S, G), np.uint8), np.zeros((S, G), np.int32)
    tused = np.zeros(S, np.int64)
    status = np.zeros(2, np.int32)
    t_full, t_con, t_dl, t_kl = np.zeros((S, C)), np.zeros((S, W, C)), np.zeros((S, G, C)), np.zeros((S, G, C))
    t_dd, t_kg = np.zeros((S, G)), np.zeros((S, G))
    const_bad = not (np.isfinite(fc2_w[:, :2 * H]).all() and np.isfinite(fc2_b).all())
    for s in range(S):
        for g in range(G):
            present[s, g] = int((live[s] & (group[s] == g)).sum())
        t_given = None if target is None else int(target[s])
        if const_bad or not (np.isfinite(state[s]).all() and np.isfinite(coef[s]).all() and np.isfinite(ego[s]).all()):
            for a in (full, con, e_all, dl, kl, dd, kg):
                a[s] = np.nan
            tused[s] = -1 if t_given is None else t_given
            status[1] += 1
            continue
        t = state[s].astype(dt) @ wp.T                                  # [W, C]
        A_t = np.abs(state[s]).astype(np.float64) @ np.abs(wp).astype(np.float64).T
        cf = coef[s].astype(dt)
        con[s] = cf[:, None] * t / dt(W)
        A_con = np.abs(coef[s]).astype(np.float64)[:, None] * A_t / W
        t_con[s] = (H + 2) * U * A_con + TINY
        e = fc2_b.astype(dt) + ego[s].astype(dt) @ we.T
        A_e = np.abs(fc2_b).astype(np.float64) + np.abs(ego[s]).astype(np.float64) @ np.abs(we).astype(np.float64).T
        e_all[s] = e

        def vector(members, rho):
            """-> (x [C], tol [C])"""
            if rho == 0:
                return e.copy(), (H + 2) * U * A_e + TINY
            x = e + dt(rho) * con[s][members].sum(axis=0)
            return x, U * ((H + 5 * W + 6) * abs(float(rho)) * A_con[members].sum(axis=0) + (H + 2) * A_e) + TINY

        full[s], t_full[s] = vector(np.ones(W, bool), dt(1))
        t_row = int(np.argmax(full[s])) if t_given is None else t_given
        tused[s] = t_row
        t_ok = 0 <= t_row < C
        if not t_ok:
            status[0] += 1
        lv, w_s = live[s], wv[s].astype(dt)
        Om, K = w_s[lv].sum(), cf[lv].sum()

        def factor(sel):
            """rho of the live members `sel`, 0 where the pooled part is zero"""
            if not sel.any() or (renorm and not cf[sel].sum() > 0):
                return dt(0)
            return (Om / w_s[sel].sum() if norm == NORM_SUM else dt(1)) * (K / cf[sel].sum() if renorm else dt(1))

        if t_ok:
            lp_full, lse_full = _lp(full[s], t_row)
            lp_e, lse_e = _lp(e, t_row)
            tl_full = 2 * t_full[s].max() + lse_abs(C) + U * float(abs(lse_full) + abs(lp_full))
            tl_e = 2 * ((H + 2) * U * A_e).max() + lse_abs(C) + U * float(abs(lse_e) + abs(lp_e))
        for g in range(G):
            R = lv & (group[s] == g)
            rest = lv & ~R
            if not R.any():
                rd, dsel = dt(1), np.ones(W, bool)
            else:
                rd, dsel = factor(rest), rest
            rk = factor(R)
            rho_d[s, g], rho_k[s, g] = float(rd), float(rk)
            dl[s, g], t_dl[s, g] = vector(dsel, rd)
            kl[s, g], t_kl[s, g] = vector(R, rk)
            if t_ok:
                lp_d, lse_d = _lp(dl[s, g], t_row)
                lp_k, lse_k = _lp(kl[s, g], t_row)
                dd[s, g], kg[s, g] = lp_full - lp_d, lp_k - lp_e
                t_dd[s, g] = (tl_full + 2 * t_dl[s, g].max() + lse_abs(C) + U * float(abs(lse_d) + abs(lp_d))
                              + U * float(abs(dd[s, g])) + TINY)
                t_kg[s, g] = (tl_e + 2 * t_kl[s, g].max() + lse_abs(C) + U * float(abs(lse_k) + abs(lp_k))
                              + U * float(abs(kg[s, g])) + TINY)
                flip[s, g] = present[s, g] > 0 and int(np.argmax(dl[s, g])) != int(np.argmax(full[s]))
    tol = dict(full=t_full, contribution=t_con, drop_logits=t_dl, keep_logits=t_kl, drop_delta=t_dd, keep_gain=t_kg)
    return Result(full, con, dl, kl, dd, kg, flip, present, tused, status, e_all, rho_d, rho_k, tol)


def member_states(variant, params, X, ids, codes, sel, W, L):
    """the oracle's final hidden states in encode()'s member order, float64 [S, W, H] (as weighted_pool_ref.forward orders
    them: pooling group, then member)"""
    import torch
    from oracle import pagg_oracle as po
    _, it = po.forward(variant, params, X, ids, codes, sel, W, L, dtype=torch.float64, return_intermediates=True)
    S = len(sel)
    _, _, group, member, _ = po.plan(variant, np.asarray(ids), np.asarray(codes), S, W, L)
    order = np.argsort(group * W + member, kind="stable")
    h = it["h"].detach().numpy()
    return h[order].reshape(S, W, h.shape[1])


def f32(a):
    return np.asarray(a).astype(np.float32)


def min_gap(res):
    """the smallest distance of two logits of one vector among full and every drop_g (what argmax and flip hang on)"""
    gaps = [np.inf]
    for x in (res.full, res.drop_logits):
        x = np.asarray(x, np.float64)
        x = x[np.isfinite(x).all(axis=-1)]
        if x.shape[-1] > 1 and x.size:
            gaps.append(np.diff(np.sort(x, axis=-1), axis=-1).min())
    return float(min(gaps))


def new_totals(G, dtype=np.float64):
    return Totals(np.zeros(G, np.int64), np.zeros(G, np.int64), np.zeros(G, np.int64), np.zeros(G, dtype), np.zeros(G, dtype))


def totals_add(tot, drop_delta, keep_gain, flip, present, rows=None):
    """pn_explain_totals: one call, in place; rows in ascending position, one addition into the running total per call"""
    dd, kg = np.asarray(drop_delta, np.float32), np.asarray(keep_gain, np.float32)
    S, G = dd.shape
    dt = tot.drop_delta_sum.dtype
    order = np.arange(S) if rows is None else np.asarray(rows, np.int64)
    order = order[(order >= 0) & (order < S)]
    for g in range(G):
        a = b = dt.type(0)
        for r in order:
            if present[r, g] > 0 and np.isfinite(dd[r, g]) and np.isfinite(kg[r, g]):
                a, b = a + dt.type(dd[r, g]), b + dt.type(kg[r, g])
                tot.rows_present[g] += 1
                tot.members[g] += int(present[r, g])
                tot.flips[g] += int(flip[r, g] != 0)
        tot.drop_delta_sum[g] += a
        tot.keep_gain_sum[g] += b
    return tot


def tol_totals(abs_sum, n):
    """bound of a running sum of n values whose absolute values sum to abs_sum"""
    return max(n, 1) * U * np.asarray(abs_sum, np.float64) + TINY


def route(S, W, H, C, G):
    """the documented work split -> [route, lanes, class chunk, H tile], for the comparison with pn_explain_route"""
    lanes = 8 if C <= 8 else 16 if C <= 16 else 64
    Cc = min(C, MAX_CON // (W + 1))
    per = W + 1 + 2 * Cc
    Ht = 1
    while Ht < H and per * ((Ht + 1) | 1) <= TILE_FLOATS:
        Ht += 1
    if Ht < H and Ht >= 4:
        Ht &= ~3
    return [ROUTE_NONE if S == 0 else ROUTE_ROW if Cc == C else ROUTE_CHUNKED, lanes, Cc, Ht]


# ---- inputs ----------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", ("state", "coef", "ego", "fc2_w", "fc2_b", "weight", "group", "G", "norm", "renorm",
                                       "target"))


def make_case(S, W, H, C, G, seed, norm=NORM_SUM, renorm=0, weights=True, target=True, gap=1e-3):
    """Random inputs whose full and drop logits are nowhere closer than `gap` to each other in the fp64 restatement: rows that
    miss are drawn again.  Group ids include -1 and G (no group); with weights, dead members of every kind.  renorm: the
    coefficients are non-negative (softmax weights), as the bounds assume."""
    rng = np.random.default_rng(seed)
    scale = max(1.0, C / 8.0)       # spreads the logits of a wide classifier, so that a gap is to be had
    fc2_w = (rng.standard_normal((C, 2 * H)) * scale / np.sqrt(H)).astype(np.float32)
    fc2_b = (rng.standard_normal(C) * scale).astype(np.float32)

    def draw(n):
        st = np.tanh(rng.standard_normal((n, W, H))).astype(np.float32)
        cf = (rng.random((n, W)) * 2 if renorm else 1 + 0.5 * rng.standard_normal((n, W))).astype(np.float32)
        eg = rng.standard_normal((n, H)).astype(np.float32)
        gr = rng.integers(-1, G + 1, size=(n, W)).astype(np.int32)
        wt = None
        if weights:
            wt = (rng.random((n, W)) * 3 + 0.25).astype(np.float32)
            dead = rng.random((n, W)) < 0.2
            wt[dead] = rng.choice(np.array([0.0, -1.0, np.nan, np.inf], np.float32), size=int(dead.sum()))
        return st, cf, eg, gr, wt

    state, coef, ego, group, weight = draw(S)
    tgt = rng.integers(0, C, size=S).astype(np.int64) if target else None
    for _ in range(200):
        if S == 0 or C == 1:
            break
        res = groups(state, coef, ego, fc2_w, fc2_b, weight, group, G, norm, renorm, tgt)
        x = np.concatenate([res.full[:, None, :], res.drop_logits], axis=1)
        miss = np.flatnonzero(np.diff(np.sort(x, axis=-1), axis=-1).min(axis=(1, 2)) < gap)
        if not len(miss):
            break
        st, cf, eg, gr, wt = draw(len(miss))
        state[miss], coef[miss], ego[miss], group[miss] = st, cf, eg, gr
        if weights:
            weight[miss] = wt
    else:
        raise AssertionError("make_case(%r): rows without a gap remain" % ((S, W, H, C, G, seed),))
    return Case(state, coef, ego, fc2_w, fc2_b, weight, group, G, norm, renorm, tgt)


def run(case, dtype=np.float64):
    return groups(*case[:6], case.group, case.G, case.norm, case.renorm, case.target, dtype=dtype)


# ---- the shapes of tests/test_gpu_explain_kernel.py: one sweep per axis around the base, then both sides of every boundary ----
BASE = dict(S=3, W=5, H=32, C=3, G=3)


def shape_table():
    """(S, W, H, C, G).  A workgroup owns a row, so "one more than two workgroups' worth of rows" is 3 rows; 513 rows more
    make every CU of the device take a second row."""
    out = []
    for H in (1, 31, 32, 33, 128, 257):
        out.append(dict(BASE, H=H))
    for W in (1, 2, 5, 40, 63, 64, 65, 130):
        out.append(dict(BASE, W=W))
        out.append(dict(BASE, W=W, G=W))
    for C in (1, 2, 7, 8, 9, 16, 17, 65):
        out.append(dict(BASE, C=C))
    for G in (1, 3, 70):
        out.append(dict(BASE, G=G))
    for S in (0, 1, 3, 513):
        out.append(dict(BASE, S=S))
    out += [dict(S=2, W=40, H=128, C=7, G=40),          # the hot shape: one tile (129 * 55 = 7095 floats)
            dict(S=2, W=40, H=128, C=8, G=3),           # (41 + 16) * 129 > 7168: two tiles of 124 and 4
            dict(S=2, W=40, H=257, C=16, G=3),          # tiles of 96, 96, 65
            dict(S=2, W=130, H=128, C=3, G=3),          # tiles of 48
            dict(S=2, W=130, H=33, C=31, G=4),          # (W + 1) * C = 4061: the last shape with one class chunk
            dict(S=2, W=130, H=33, C=32, G=4),          # 4192 > 4096: chunks of 31 and 1
            dict(S=2, W=130, H=33, C=65, G=4),          # chunks of 31, 31, 3
            dict(S=2, W=5, H=32, C=3, G=1024)]          # more than 64 KB of LDS
    seen, uniq = set(), []
    for sh in out:
        key = tuple(sorted(sh.items()))
        if key not in seen:
            seen.add(key)
            uniq.append(sh)
    return uniq
