"""NumPy restatement of pn_explain_units / pn_explain_overlap / pn_explain_node_totals (include/pathnet_hip.h).  Nothing here
runs on a GPU.

Units are np.unique per row.  The overlap result for unit g is explain_ref.groups(...) called with the PARTITION
group = where(member touches g, 0, -1), G = 1, column 0: the kernel's sums for one g are exactly those of that call (the same
members in the same ascending order, the same factors), so its `tol` is the bound and no new error analysis is needed.
Discrete outputs are compared exactly.
"""
import collections

import numpy as np

import explain_ref as ref

UNIT_NODE, UNIT_EDGE = 0, 1
NO_KEY = np.int64(-1)


def edge_key(a, b):
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return (np.minimum(a, b) << 32) | np.maximum(a, b)


def edge_ends(key):
    key = np.asarray(key, np.int64)
    return np.stack([key >> 32, key & 0xFFFFFFFF], -1)


def keys(node, kind, exclude=None):
    """node int [S, W, L] -> int64 [S, W, M], -1 where the step has no unit"""
    node = np.asarray(node, np.int64)
    if kind == UNIT_NODE:
        k = node.copy()
        bad = node < 0
        if exclude is not None:
            bad |= node == np.asarray(exclude, np.int64)[:, None, None]
    else:
        assert exclude is None
        a, b = node[:, :, :-1], node[:, :, 1:]
        k = edge_key(a, b)
        bad = (a < 0) | (b < 0)
    return np.where(bad, NO_KEY, k)


def units(node, kind, exclude=None):
    """pn_explain_units -> (unit int64 [S, W * M], count int32 [S], label int32 [S, W, M])"""
    k = keys(node, kind, exclude)
    S, W, M = k.shape
    unit = np.full((S, W * M), -1, np.int64)
    count = np.zeros(S, np.int32)
    label = np.full((S, W, M), -1, np.int32)
    for s in range(S):
        u = np.unique(k[s][k[s] >= 0])
        count[s] = len(u)
        unit[s, :len(u)] = u
        ok = k[s] >= 0
        label[s][ok] = np.searchsorted(u, k[s][ok])
    return unit, count, label


def touches(label, G):
    """label int [S, W, M] -> bool [S, G, W]: member j carries label g (a label outside [0, G) is no membership)"""
    label = np.asarray(label, np.int64)
    S, W, M = label.shape
    out = np.zeros((S, G, W), bool)
    s, j, m = np.nonzero((label >= 0) & (label < G))
    out[s, label[s, j, m], j] = True
    return out


SCALAR = ("drop_delta", "keep_gain", "flip", "present")
VECTOR = ("drop_logits", "keep_logits")


def overlap(state, coef, ego, fc2_w, fc2_b, weight, label, G, norm, renorm, target=None, dtype=np.float64, in_dtype=np.float32):
    """pn_explain_overlap -> explain_ref.Result with G columns: column g is explain_ref.groups of the partition
    {members that touch g} | {the rest: no group}; full, contribution, target_used, status and e are those of any one call"""
    label = np.asarray(label)
    S, W, M = label.shape
    tch = touches(label, G)
    cols = [ref.groups(state, coef, ego, fc2_w, fc2_b, weight, np.where(tch[:, g], 0, -1), 1, norm, renorm, target, dtype=dtype,
                       in_dtype=in_dtype) for g in range(G)]
    first = cols[0]
    cat = lambda k: np.concatenate([getattr(c, k) for c in cols], axis=1)          # noqa: E731
    tol = dict(first.tol)
    for k in SCALAR[:2] + VECTOR:
        tol[k] = np.concatenate([c.tol[k] for c in cols], axis=1)
    return ref.Result(first.full, first.contribution, cat("drop_logits"), cat("keep_logits"), cat("drop_delta"), cat("keep_gain"),
                      cat("flip"), cat("present"), first.target_used, first.status, first.e, cat("rho_d"), cat("rho_k"), tol)


NodeTable = collections.namedtuple("NodeTable", ("rows_present", "members", "flips", "top"))


def new_table(N):
    return NodeTable(*(np.zeros(N, np.int64) for _ in range(4)))


def node_totals_add(tab, unit, drop_delta, keep_gain, flip, present, rows=None):
    """pn_explain_node_totals: one call, in place"""
    dd, kg = np.asarray(drop_delta, np.float32), np.asarray(keep_gain, np.float32)
    unit = np.asarray(unit, np.int64)
    S, G = dd.shape
    N = len(tab.rows_present)
    order = np.arange(S) if rows is None else np.asarray(rows, np.int64)
    for r in order[(order >= 0) & (order < S)]:
        ok = (present[r] > 0) & np.isfinite(dd[r]) & np.isfinite(kg[r]) & (unit[r] >= 0) & (unit[r] < N)
        g = np.flatnonzero(ok)
        np.add.at(tab.rows_present, unit[r, g], 1)
        np.add.at(tab.members, unit[r, g], np.asarray(present)[r, g].astype(np.int64))
        np.add.at(tab.flips, unit[r, g], (np.asarray(flip)[r, g] != 0).astype(np.int64))
        if len(g):
            tab.top[unit[r, g[np.argmax(dd[r, g])]]] += 1          # (argmax: the first of equals)
    return tab


# ---- inputs ----------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", ref.Case._fields[:6] + ("label", "G", "M", "norm", "renorm", "target"))
GAP = 1e-5          # a row has up to W * M drop vectors: explain_ref's 1e-3 would reject most rows; still >= 1e5 x the logit bound


def make_case(S, W, H, C, G, M, seed, norm=ref.NORM_SUM, renorm=0, weights=True, target=True, label_lo=-1, label_hi=None,
              hub=False, redraws=None):
    """explain_ref.make_case with labels [S, W, M] drawn from [label_lo, label_hi] (default -1 .. G: both are "no group").
    hub: unit 0 sits on every member.  Rows whose full or drop logits come closer than GAP are drawn again; at most 200 times
    (asserted).  redraws: a list that receives the number of redraws."""
    rng = np.random.default_rng(seed)
    hi = G if label_hi is None else label_hi
    scale = max(1.0, C / 8.0)
    fc2_w = (rng.standard_normal((C, 2 * H)) * scale / np.sqrt(H)).astype(np.float32)
    fc2_b = (rng.standard_normal(C) * scale).astype(np.float32)

    def draw(n):
        st = np.tanh(rng.standard_normal((n, W, H))).astype(np.float32)
        cf = (rng.random((n, W)) * 2 if renorm else 1 + 0.5 * rng.standard_normal((n, W))).astype(np.float32)
        eg = rng.standard_normal((n, H)).astype(np.float32)
        lb = rng.integers(label_lo, hi + 1, size=(n, W, M)).astype(np.int32)
        if hub:
            lb[:, :, 0] = 0
        wt = None
        if weights:
            wt = (rng.random((n, W)) * 3 + 0.25).astype(np.float32)
            dead = rng.random((n, W)) < 0.2
            wt[dead] = rng.choice(np.array([0.0, -1.0, np.nan, np.inf], np.float32), size=int(dead.sum()))
        return st, cf, eg, lb, wt

    state, coef, ego, label, weight = draw(S)
    tgt = rng.integers(0, C, size=S).astype(np.int64) if target else None
    todo = np.arange(S)
    n_redraws = 0
    while len(todo) and C > 1:
        w = None if weight is None else weight[todo]
        res = overlap(state[todo], coef[todo], ego[todo], fc2_w, fc2_b, w, label[todo], G, norm, renorm,
                      None if tgt is None else tgt[todo])
        x = np.concatenate([res.full[:, None, :], res.drop_logits], axis=1)
        miss = todo[np.diff(np.sort(x, axis=-1), axis=-1).min(axis=(1, 2)) < GAP]
        if not len(miss):
            break
        n_redraws += 1
        assert n_redraws <= 200, "make_case(%r): rows without a gap remain after 200 redraws" % ((S, W, H, C, G, M, seed),)
        st, cf, eg, lb, wt = draw(len(miss))
        state[miss], coef[miss], ego[miss], label[miss] = st, cf, eg, lb
        if weights:
            weight[miss] = wt
        todo = miss
    if redraws is not None:
        redraws.append(n_redraws)
    return Case(state, coef, ego, fc2_w, fc2_b, weight, label, G, M, norm, renorm, tgt)


def run(case, dtype=np.float64):
    return overlap(*case[:6], case.label, case.G, case.norm, case.renorm, case.target, dtype=dtype)
