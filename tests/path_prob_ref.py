"""CPU reference of the path likelihoods (pn_path_prob, pathnet_amd/pathprob.py) in Python integers and fractions, kept
independent of the library's thresholds.

Tables are the dicts of biased_ref.merw_tables / uniform_tables: off, A, B, S from oracle.merw.alias_build (or
sampler.build_uniform) and the directed edges (eu, ev) of the hop source.  The walker's step is
    slot = r0 % k,   next = (1.0 * r1 / RAND_MAX > S[slot]) ? A[slot] : B[slot],   r0, r1 uniform on [0, 2^31),
so  N(cur -> x) = sum_s c_s * (cntA_s [A_s == x] + cntB_s [B_s == x])  over 2^62, with c_s = 2^31 // k + (s < 2^31 % k) the
draws that select slot s and cntA_s the number of r1 that satisfy the predicate -- found here by bisection on the fp64
predicate itself (it is monotone in r1), not from the library's thr.
Classes come from the set of directed edges; realised and target probabilities are exact fractions.
"""
import functools
from fractions import Fraction

import numpy as np

import biased_ref

TWO31, TWO32, TWO62 = 2 ** 31, 2 ** 32, 2 ** 62
RAND_MAX = 2147483647.0
TRIALS = biased_ref.MAX_TRIALS


@functools.lru_cache(None)
def count_a(s):
    """the number of r in [0, 2^31) with 1.0 * r / RAND_MAX > s"""
    if not 1.0 * (TWO31 - 1) / RAND_MAX > s:
        return 0
    lo, hi = 0, TWO31 - 1           # the predicate holds at hi
    while lo < hi:
        mid = (lo + hi) // 2
        if 1.0 * mid / RAND_MAX > s:
            hi = mid
        else:
            lo = mid + 1
    return TWO31 - lo


def node_numerators(tb, cur):
    """{x: N(cur -> x)} of one node; empty for an empty table"""
    cache = tb.setdefault("_num", {})
    if cur not in cache:
        o0, o1 = int(tb["off"][cur]), int(tb["off"][cur + 1])
        k = o1 - o0
        got = {}
        for s in range(k):
            c = TWO31 // k + (1 if s < TWO31 % k else 0)
            na = count_a(float(tb["S"][o0 + s]))
            a, b = int(tb["A"][o0 + s]), int(tb["B"][o0 + s])
            got[a] = got.get(a, 0) + c * na
            got[b] = got.get(b, 0) + c * (TWO31 - na)
        cache[cur] = got
    return cache[cur]


def edge_set(tb):
    if "_edges" not in tb:
        tb["_edges"] = set(zip(tb["eu"].tolist(), tb["ev"].tolist()))
    return tb["_edges"]


def node_class(tb, prev, y):
    return 0 if y == prev else (1 if (prev, y) in edge_set(tb) else 2)


def path_prob(tb, ids, second_order=False):
    """-> dict(num int64 [..., L-1], counters [4]) and, second order, mass int64 [..., L-1, 3] and cls uint8 [..., L-1]: the
    contract of pn_path_prob restated"""
    ids = np.asarray(ids)
    n, L = tb["n"], ids.shape[-1]
    flat = ids.reshape(-1, L).tolist()
    num = np.zeros((len(flat), max(L - 1, 0)), np.int64)
    mass = np.zeros((len(flat), max(L - 1, 0), 3), np.int64)
    cls = np.full((len(flat), max(L - 1, 0)), 3, np.uint8)
    counters = [0, 0, 0, 0]
    for i, path in enumerate(flat):
        for t in range(L - 1):
            cur, nxt = path[t], path[t + 1]
            bad = (not 0 <= cur < n) + (not 0 <= nxt < n)
            if bad:
                counters[0] += bad
                continue
            row = node_numerators(tb, cur)
            if int(tb["off"][cur + 1]) == int(tb["off"][cur]):
                counters[1] += 1
            elif row.get(nxt, 0) == 0:
                counters[2] += 1
            num[i, t] = row.get(nxt, 0)
            if second_order and t >= 1 and 0 <= path[t - 1] < n:
                prev = path[t - 1]
                cls[i, t] = node_class(tb, prev, nxt)
                m = [0, 0, 0]
                for y, v in row.items():
                    m[node_class(tb, prev, y)] += v
                mass[i, t] = m
    lead = ids.shape[:-1] + (max(L - 1, 0),)
    out = dict(num=num.reshape(lead), counters=np.array(counters, np.int64))
    if second_order:
        out.update(mass=mass.reshape(lead + (3,)), cls=cls.reshape(lead))
    return out


def realised(num, mass, cls, T):
    """exact probability of one transition under the biased walker: trials 1..63 accept a proposal of class c with
    probability T_c / 2^32, the 64th proposal is taken as it is.  cls == 3: the plain table step."""
    qx = Fraction(int(num), TWO62)
    if cls == 3:
        return qx
    a = [Fraction(int(t), TWO32) for t in T]
    alpha = sum(Fraction(int(m), TWO62) * a[c] for c, m in enumerate(mass))
    if alpha == 0:
        return qx
    rest = (1 - alpha) ** (TRIALS - 1)
    return qx * a[cls] * (1 - rest) / alpha + rest * qx


def target(num, mass, cls, p, q):
    """exact probability of one transition under the target distribution; p, q: numbers or inf"""
    if cls == 3:
        return Fraction(int(num), TWO62)
    w = [Fraction(0) if x == float("inf") else 1 / Fraction(x) for x in (p, 1, q)]
    den = sum(int(m) * w[c] for c, m in enumerate(mass))
    return Fraction(0) if den == 0 else int(num) * w[cls] / den


def rel_err(got, exact):
    """|got - exact| / exact as a float, for a float `got` and a Fraction `exact` > 0"""
    return float(abs(Fraction(got) - exact) / exact)
