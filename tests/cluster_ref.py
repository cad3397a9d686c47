"""NumPy fp64 restatement of pn_kmeans_* and pn_cluster_scores (pathnet_amd/csrc/pn_kmeans.hip) over the explicit [N, K] key
matrix, with the derived error bounds, tolerant checkers that leave no row out, named WRONG implementations and the input
builders of the GPU tests.  Not a test.

The definition is include/pathnet_hip.h's "clustering" section; the function names follow its entry points.  Everything the
kernels do in fp64 is restated in the kernels' ORDER (sequential sums by numpy.add.accumulate, the 64-lane butterfly, the
halving tree), so those values are expected bit for bit; the fp32 scores come from the MFMA's fma chain, which numpy cannot
restate, and are held to bounds.

The bounds.  u = 2^-24, v = 2^-53, first order, times SAFETY = 1.5 (knn_ref's derivation).
 1. cosine score.  z^ = fl32(x / norm) and m^ each carry a relative u; one k-ordered fma chain of D products on unit rows,
    D u (Cauchy-Schwarz); the rounding of the score itself and slack for the fp64 norms, 2u:       E = (D + 4) u     tol_score
 2. euclidean score.  The operands are exact; the chain alone:  E_rc = D u sum_d |z_rd m_cd|  per pair.  With integer entries
    and sum_d |z m| < 2^24 every partial sum is an integer below 2^24: the chain is EXACT.  The key subtracts h_c, an fp64 sum
    of D exact squares (D v h_c, far below the score's bound) and one rounding.
 3. a centroid coordinate.  The fp64 sum of `count` terms in any fixed order: (count - 1) v sum |z|; the division v more; the
    rounding to fp32 u |m|.  Cosine: the norm of the mean, D + 2 roundings of positive terms, moves every coordinate by
    (D + 3) v |m| more.                                                                                        tol_centroid
 4. inertia.  Each cost carries the score's bound (x 2 for euclidean: d = q - 2 e); the sum of n non-negative terms in blocks
    adds (256 + blocks) v sum d.  Given the GPU's own keys the costs are exact and only the latter remains.    tol_inertia
 5. scores.  A term of MI is (x / n) log(n x / (a b)): the argument carries 3 roundings, the log 1 ulp in each of the two
    libraries, the product and the quotient one each: |term| 5 v + (x / n) 4 v; the sum of T terms (T - 1) v sum |term|; the
    entropies alike; the quotient 2 v.  ARI: exact integers, then 5 roundings of values no larger than C(n, 2), divided by the
    denominator.  Purity: one division.                                                                          tol_nmi, tol_ari
"""
import ctypes

import numpy as np

from dropout_ref import philox4

U = 2.0 ** -24
V = 2.0 ** -53
SAFETY = 1.5
COSINE, EUCLIDEAN = 0, 1
MAX_K = 1024
STREAM = 0x4B4D
BLOCK = 256
CHUNK = 64
DBL_MAX = np.finfo(np.float64).max

VARIANTS = ("ties_high", "nonorm_centroid", "no_offset", "empty_zeroed", "dead_assigned", "chunk_edge", "stale_inertia",
            "rand_index", "nmi_geometric", "pick_ge")


class Result:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def plan(N, D, K):
    from pathnet_amd import _lib
    out = (ctypes.c_int64 * 6)()
    _lib.check(_lib.load().pn_kmeans_plan(N, D, K, out))
    return tuple(int(v) for v in out)


def workspace_bytes(N, D, K, iters=0):
    from pathnet_amd import _lib
    need = ctypes.c_int64(-1)
    _lib.check(_lib.load().pn_kmeans_workspace_bytes(N, D, K, iters, ctypes.byref(need)))
    return need.value


def r8(b):
    return (b + 7) & ~7


def workspace_formula(N, D, K, iters=0):
    """the header's text"""
    T = -(-N // 64)
    return (64 + r8(4 * (N + K) * D) + 6 * r8(4 * N) + 24 * N + 16 * K + 8 * -(-N // 256) + r8(4 * T) + r8(N) + 8 * iters
            + 2 * r8(4 * (K + 2)) + 8 * (T + K) * D + r8(20 * N) + (8 << 20))


# ---- the kernels' orders of addition ---------------------------------------------------------------------------------------------
def seq_sum(v, axis=-1):
    """one adder, ascending"""
    v = np.asarray(v, np.float64)
    if v.shape[axis] == 0:
        return np.zeros(np.delete(v.shape, axis))
    return np.take(np.add.accumulate(v, axis=axis), -1, axis=axis)


def lane_sum(P):
    """[n, D] -> [n]: per residue of d mod 64 in ascending d, then the xor butterfly 32 .. 1 (every lane ends with the same
    value: lane 0's is taken)"""
    P = np.asarray(P, np.float64)
    n, D = P.shape
    pad = -D % 64
    lanes = seq_sum(np.concatenate((P, np.zeros((n, pad))), axis=1).reshape(n, -1, 64), axis=1)
    idx = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, idx ^ m]
    return lanes[:, 0]


def blocked_sum(v):
    """blocks of 256 in ascending order, then the block sums in ascending order -> (total, block sums)"""
    v = np.asarray(v, np.float64)
    nb = -(-len(v) // BLOCK)
    bs = np.array([seq_sum(v[b * BLOCK:(b + 1) * BLOCK]) for b in range(nb)], np.float64)
    return (float(seq_sum(bs)) if nb else 0.0), bs


# ---- prepare ------------------------------------------------------------------------------------------------------------------------
def prepare(X, metric, valid=None):
    """-> Result(live [N] bool, z [N, D] fp32 prepared rows, q [N] fp64, dead)"""
    X = np.asarray(X, np.float32)
    N, D = X.shape
    x = X.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        fin = np.isfinite(x).all(axis=1)
        xz = np.where(fin[:, None], x, 0.0)
        norm = np.sqrt(lane_sum(xz * xz)) if N else np.zeros(0)
        ok = fin & ((metric == EUCLIDEAN) | ((norm > 0) & (norm <= DBL_MAX)))
        live = ok & (np.ones(N, bool) if valid is None else np.asarray(valid).reshape(-1) != 0)
        if metric == COSINE:
            z = (xz / np.where(live, norm, 1.0)[:, None]).astype(np.float32)
        else:
            z = X.copy()
        z[~live] = 0
        q = seq_sum(xz * xz, axis=1) if metric == EUCLIDEAN else np.zeros(N)
        q = np.where(live, q, 0.0)
    return Result(N=N, D=D, metric=metric, live=live, z=z, q=q, dead=int((~live).sum()))


def offsets(m, metric):
    """h [K] fp64: +inf for a centroid that is not live"""
    m64 = np.asarray(m, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        fin = np.isfinite(m64).all(axis=1)
        ss = seq_sum(np.where(fin[:, None], m64, 0.0) ** 2, axis=1)
    ok = fin & ((metric == EUCLIDEAN) | (ss > 0))
    return np.where(ok, 0.5 * ss if metric == EUCLIDEAN else 0.0, np.inf)


# ---- assign -------------------------------------------------------------------------------------------------------------------------
def keys(p, m, variant=None):
    """-> (e [N, K] fp64 keys from the fp64 scores rounded to fp32, E [N, K] the bound per pair)"""
    z64, m64 = p.z.astype(np.float64), np.asarray(m, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (z64 @ m64.T).astype(np.float32)
        s = np.where(np.isnan(s), -np.inf, s).astype(np.float64)
        h = offsets(m, p.metric)
        if variant == "no_offset":
            h = np.where(np.isfinite(h), 0.0, h)
        e = np.where(np.isinf(h)[None, :], -np.inf, s - np.where(np.isinf(h), 0.0, h)[None, :])
        if p.metric == COSINE:
            E = np.full(e.shape, SAFETY * (p.D + 4) * U)
        else:
            E = SAFETY * p.D * U * (np.abs(z64) @ np.abs(np.where(np.isfinite(m64), m64, 0.0)).T)
    return e, E


def costs(p, key):
    with np.errstate(invalid="ignore"):
        d = p.q - 2.0 * key if p.metric == EUCLIDEAN else 1.0 - key
        d = np.where(d > 0, d, 0.0)
    return np.where(p.live, d, 0.0)


def assign(p, m, prev=None, variant=None, stale=None):
    """-> Result(label int64 [N], key [N], cost [N], moved, inertia, e, E)"""
    e, E = keys(p, m, variant)
    K = e.shape[1]
    if variant == "ties_high":
        label = (K - 1 - np.argmax(e[:, ::-1], axis=1)).astype(np.int64)
    else:
        label = np.argmax(e, axis=1).astype(np.int64) if p.N else np.zeros(0, np.int64)
    key = e[np.arange(p.N), label] if p.N else np.zeros(0)
    alive = np.ones(p.N, bool) if variant == "dead_assigned" else p.live
    label = np.where(alive, label, -1)
    key = np.where(alive, key, -np.inf)
    cost = costs(p, key)
    moved = int((p.live & (label != (label + 1 if prev is None else np.asarray(prev)))).sum())
    inertia = blocked_sum(cost)[0]
    if variant == "stale_inertia" and stale is not None:        # the costs against the PREVIOUS centroids
        es, _ = keys(p, stale)
        inertia = blocked_sum(costs(p, np.where(p.live, es[np.arange(p.N), np.maximum(label, 0)], -np.inf)))[0]
    return Result(label=label, key=key, cost=cost, moved=moved, inertia=inertia, e=e, E=E)


def check_assign(got_label, got_key, p, m, exact=False):
    """None when every row's label and key are acceptable, else a string naming the first row that is not.  A label is
    accepted if its true key is within twice the bound of the true maximum; the key if it is within the bound of that
    label's true key.  Dead rows: -1 and -inf.  No row is left out.  exact (integer inputs with sum |z m| < 2^24, where the
    chain is exact): labels and keys must be the restatement's, ties included, bit for bit."""
    if exact:
        a = assign(p, m)
        bad = np.flatnonzero((np.asarray(got_label) != a.label) | (np.asarray(got_key, np.float64).view(np.int64) !=
                                                                   (a.key + 0.0).view(np.int64)))
        return None if not len(bad) else "row %d: label %d key %r, expected %d and %r" % (
            bad[0], got_label[bad[0]], got_key[bad[0]], a.label[bad[0]], a.key[bad[0]])
    z64, m64 = p.z.astype(np.float64), np.asarray(m, np.float32).astype(np.float64)
    h = offsets(m, p.metric)
    with np.errstate(invalid="ignore", over="ignore"):
        true = np.where(np.isinf(h)[None, :], -np.inf, z64 @ np.where(np.isfinite(m64), m64, 0.0).T - np.where(np.isinf(h), 0.0, h))
    _, E = keys(p, m)
    for r in range(p.N):
        lab, key = int(got_label[r]), float(got_key[r])
        if not p.live[r]:
            if lab != -1 or key != -np.inf:
                return "dead row %d: label %d key %r" % (r, lab, key)
            continue
        if not 0 <= lab < len(h):
            return "row %d: label %d" % (r, lab)
        best = true[r].max()
        if np.isfinite(best):
            if not true[r, lab] >= best - 2 * E[r].max():
                return "row %d: label %d has key %r, the maximum is %r (bound %g)" % (r, lab, true[r, lab], best, E[r].max())
            if not abs(key - true[r, lab]) <= E[r, lab] + 4 * V * abs(h[lab]):
                return "row %d: key %r, true %r (bound %g)" % (r, key, true[r, lab], E[r, lab])
        elif key != best and not (np.isinf(key) and np.isinf(best)):
            return "row %d: key %r, true %r" % (r, key, best)
    return None


def tol_inertia(cost):
    """given the keys: the sum's own rounding"""
    n = len(cost)
    return SAFETY * (BLOCK + -(-n // BLOCK)) * V * float(np.abs(cost).sum())


def tol_inertia_scores(p, a):
    """given the labels only: every cost also carries its score's bound (twice for euclidean, d = q - 2 e)"""
    rows = np.flatnonzero(np.asarray(a.label) >= 0)
    return (2.0 if p.metric == EUCLIDEAN else 1.0) * float(a.E[rows, np.asarray(a.label)[rows]].sum()) + tol_inertia(a.cost)


# ---- update -------------------------------------------------------------------------------------------------------------------------
def update(p, label, prev_m, variant=None):
    """-> Result(m fp32 [K, D], count int64 [K], empty, sums fp64 [K, D], abs fp64 [K, D] = sum |z|)"""
    prev_m = np.asarray(prev_m, np.float32)
    K, D = prev_m.shape
    label = np.asarray(label, np.int64)
    lab = np.where(p.live & (label >= 0) & (label < K), label, K)
    order = np.argsort(lab, kind="stable")
    off = np.searchsorted(lab[order], np.arange(K + 2))
    z64 = p.z.astype(np.float64)
    m, count, empty = prev_m.copy(), np.zeros(K, np.int64), 0
    sums, mags = np.zeros((K, D)), np.zeros((K, D))
    for c in range(K):
        rows = order[off[c]:off[c + 1]]
        count[c] = len(rows)
        if variant == "chunk_edge" and len(rows) > CHUNK and c + 1 < K:      # a chunk's last member goes to the next cluster
            rows = np.delete(rows, CHUNK - 1)
        if count[c] == 0:
            empty += 1
            if variant == "empty_zeroed":
                m[c] = 0
            continue
        parts = [seq_sum(z64[rows[i:i + CHUNK]], axis=0) for i in range(0, len(rows), CHUNK)]
        sums[c] = seq_sum(np.stack(parts), axis=0)
        mags[c] = np.abs(z64[rows]).sum(axis=0)
        mean = sums[c] / float(count[c])
        if p.metric == EUCLIDEAN or variant == "nonorm_centroid":
            m[c] = mean.astype(np.float32)
            continue
        sq = mean * mean
        red = seq_sum(np.concatenate((sq, np.zeros(-D % 256))).reshape(-1, 256), axis=0)
        s = 128
        while s >= 1:
            red[:s] = red[:s] + red[s:2 * s]
            s //= 2
        nrm = np.sqrt(red[0])
        if not (nrm > 0 and nrm <= DBL_MAX):
            empty += 1
            continue
        m[c] = (mean / nrm).astype(np.float32)
    return Result(m=m, count=count, empty=empty, sums=sums, mags=mags)


def tol_centroid(p, ref):
    """[K, D]: the bound on a coordinate of the new centroid (0 where the cluster keeps its centroid)"""
    cnt = np.maximum(ref.count, 1)[:, None].astype(np.float64)
    a = np.abs(ref.m.astype(np.float64))
    tol = (cnt - 1) * V * ref.mags / cnt + 2 * V * a + U * a
    if p.metric == COSINE:
        mean = np.abs(ref.sums) / cnt
        nrm = np.sqrt((mean ** 2).sum(axis=1, keepdims=True))
        tol = tol / np.where(nrm > 0, nrm, 1.0) + (p.D + 3) * V * a
    return SAFETY * tol


def check_update(got_m, got_count, got_empty, p, label, prev_m):
    """None when the centroids, counts and the empty count are acceptable GIVEN these labels, else a string"""
    ref = update(p, label, prev_m)
    if not (np.asarray(got_count) == ref.count).all():
        return "counts %s, expected %s" % (np.asarray(got_count)[:8], ref.count[:8])
    if int(got_empty) != ref.empty:
        return "empty %d, expected %d" % (int(got_empty), ref.empty)
    diff = np.abs(np.asarray(got_m, np.float64) - ref.m.astype(np.float64))
    bad = np.argwhere(~(diff <= tol_centroid(p, ref)))
    if len(bad):
        c, d = bad[0]
        return "centroid [%d, %d] = %r, expected %r (bound %g)" % (c, d, got_m[c][d], ref.m[c, d], tol_centroid(p, ref)[c, d])
    return None


# ---- k-means++ ----------------------------------------------------------------------------------------------------------------------
def draw(seed, restart, j):
    w = philox4(seed, (int(restart) << 32) | int(j), STREAM)
    r53 = ((int(w[0]) | (int(w[1]) << 32)) >> 11)
    return float(r53) * 2.0 ** -53


def distance_to(p, c):
    """d(r, chosen row c) as the seeding forms it: fp64 products and sums in the 64-lane order"""
    z64 = p.z.astype(np.float64)
    e = lane_sum(z64 * z64[c][None, :])
    if p.metric == EUCLIDEAN:
        e = e - 0.5 * p.q[c]
    return costs(p, e)


def weights_after(p, chosen):
    """the weights of the round that follows the picks `chosen` (all >= 0)"""
    if not len(chosen):
        return p.live.astype(np.float64)
    mind = np.full(p.N, np.inf)
    for c in chosen:
        mind = np.minimum(mind, distance_to(p, int(c)))
    return np.where(p.live, mind, 0.0)


def prefix(w):
    """P_r in the two-level order -> (P [N], P_total)"""
    total, bs = blocked_sum(w)
    base = np.concatenate(([0.0], np.add.accumulate(bs)))[:-1] if len(bs) else np.zeros(0)
    P = np.concatenate([base[b] + np.add.accumulate(w[b * BLOCK:(b + 1) * BLOCK]) for b in range(len(bs))]) if len(bs) else w
    return P, total


def pick(p, w, taken, seed, restart, j, variant=None, draw=draw):
    P, total = prefix(w)
    if total > 0 and total <= DBL_MAX:
        t = draw(seed, restart, j) * total
        hit = np.flatnonzero(P >= t if variant == "pick_ge" else P > t)
        return int(hit[0]) if len(hit) else int(np.flatnonzero(w > 0)[-1])
    free = np.flatnonzero(p.live & ~taken)
    if len(free):
        return int(free[0])
    alive = np.flatnonzero(p.live)
    return int(alive[0]) if len(alive) else -1


def seed_centroids(p, K, seed, restart, variant=None, draw=draw):
    """-> (chosen int64 [K], centroids fp32 [K, D]).  draw: the uniform number of (seed, restart, round), replaceable so that
    a test can land t on a prefix sum"""
    chosen, taken = [], np.zeros(p.N, bool)
    mind = np.full(p.N, np.inf)
    for j in range(K):
        if j == 0:
            w = p.live.astype(np.float64)
        elif chosen[-1] >= 0:
            mind = np.minimum(mind, distance_to(p, chosen[-1]))
            w = np.where(p.live, mind, 0.0)
        else:
            w = np.zeros(p.N)
        c = pick(p, w, taken, seed, restart, j, variant, draw)
        if c >= 0:
            taken[c] = True
        chosen.append(c)
    chosen = np.array(chosen, np.int64)
    m = np.where((chosen >= 0)[:, None], p.z[np.maximum(chosen, 0)], np.float32(0)) if p.N else np.zeros((K, p.D), np.float32)
    return chosen, m.astype(np.float32)


def check_seed(got_chosen, got_m, p, K, seed, restart, draw=draw):
    """Replays every round from the GPU's OWN earlier picks: pick j is accepted if t lies in the picked row's prefix interval
    [P_{r-1}, P_r) widened by the prefix bound (r + 2) v P_r -- the weights themselves are restated in the kernel's order; with
    integer weights the prefix sums are exact and nothing is widened.  No pick is left out.  None or a string."""
    got_chosen = np.asarray(got_chosen, np.int64)
    taken = np.zeros(p.N, bool)
    for j in range(K):
        c = int(got_chosen[j])
        w = weights_after(p, got_chosen[:j]) if (j == 0 or (got_chosen[:j] >= 0).all()) else np.zeros(p.N)
        P, total = prefix(w)
        if total > 0 and total <= DBL_MAX:
            t = draw(seed, restart, j) * total
            if not 0 <= c < p.N or not w[c] > 0:
                return "pick %d: row %d has no weight" % (j, c)
            tol = 0.0 if (w == np.rint(w)).all() and total < 2.0 ** 53 else SAFETY * (c + 2) * V * P[c]
            below = P[c - 1] if c > 0 else 0.0
            if not (below - tol <= t < P[c] + tol):
                return "pick %d: row %d, t = %r outside [%r, %r)" % (j, c, t, below, P[c])
        else:
            want = pick(p, w, taken, seed, restart, j, None, draw)
            if c != want:
                return "pick %d: row %d, the fallback order gives %d" % (j, c, want)
        if c >= 0:
            taken[c] = True
        want_m = p.z[c] if c >= 0 else np.zeros(p.D, np.float32)
        if not (np.asarray(got_m[j]).view(np.uint32) == want_m.view(np.uint32)).all():
            return "centroid %d is not prepared row %d" % (j, c)
    return None


# ---- the loop -----------------------------------------------------------------------------------------------------------------------
def lead(a):
    """the smallest lead of a live row's best key over any other, in units of the pair bounds (inf with one cluster)"""
    e, E = a.e, a.E
    N, K = e.shape
    if K < 2 or not N:
        return np.inf
    rows = np.arange(N)
    best = np.maximum(a.label, 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = (e[rows, best][:, None] - e) / np.maximum(E[rows, best][:, None], E)
    gap[rows, best] = np.inf
    gap = gap[np.asarray(a.label) >= 0]
    return float(gap.min()) if gap.size else np.inf


def run(X, K, metric, iters, restarts=1, seed=0, init=None, valid=None, variant=None):
    """pn_kmeans_run -> Result(label, centroid, count, inertia, iterations, moved [iters], restart, dead, lead: the smallest
    lead over every assignment of every restart, chosen [restarts, K])"""
    p = prepare(X, metric, valid)
    best, worst, picks, inertias, tols = None, np.inf, [], [], []
    for rho in range(restarts):
        if init is not None:
            m, chosen = np.asarray(init, np.float32).copy(), np.full(K, -1, np.int64)
        else:
            chosen, m = seed_centroids(p, K, seed, rho, variant)
        picks.append(chosen)
        moved, prev, its, a, upd = np.full(iters, -1, np.int64), None, 0, None, None
        for t in range(iters):
            a = assign(p, m, prev, variant)
            worst = min(worst, lead(a))
            moved[t], prev, its = a.moved, a.label, its + 1
            if a.moved == 0:
                break
            if t + 1 < iters:
                upd = update(p, a.label, m, variant)
                m = upd.m
        cur = Result(label=a.label, centroid=m, update=upd, inertia=a.inertia, iterations=its, moved=moved, restart=rho,
                     count=np.bincount(a.label[a.label >= 0], minlength=K).astype(np.int64))
        inertias.append(a.inertia)
        tols.append(tol_inertia_scores(p, a))
        cur.tol_inertia = tols[-1]
        if best is None or (np.isfinite(cur.inertia) and (not np.isfinite(best.inertia) or cur.inertia < best.inertia)):
            best = cur
    best.dead, best.lead, best.chosen, best.p = p.dead, worst, np.stack(picks), p
    best.inertias, best.tols = np.array(inertias), np.array(tols)
    return best


def blobs(N, D, K, seed):
    """planted Gaussian blobs: centres N(0, 16 I), unit noise, fp32 -> (X [N, D], the planted cluster of every row)"""
    rng = np.random.default_rng(seed)
    centres = 4.0 * rng.standard_normal((K, D))
    which = rng.integers(0, K, N)
    return (centres[which] + rng.standard_normal((N, D))).astype(np.float32), which


# (shape, seeds) whose whole trajectory is decidable: every row's best key leads by LEAD bounds in every assignment
# (tests/test_cluster_ref_host.py asserts it).  (129, 33, 3) runs seeds 1 .. 3: with this stream's picks seed 0 leads by only
# 7.8 bounds under cosine and is left out for that reason, as seed 0 of (700, 40, 130) is.
DECIDABLE = [((300, 17, 5), (0, 1, 2)), ((129, 33, 3), (1, 2, 3)), ((65, 16, 2), (0, 1, 2)), ((700, 40, 130), (1, 2))]
DECIDABLE_ITERS = 12
# three restarts of which a later one wins: the blobs of (300, 17, 5), seed 1, cut into 7 clusters, 20 iterations
RESTART_CASE = ((300, 17, 5), 1, 7, 20, 3)
LEAD = 8.0


# ---- scores -------------------------------------------------------------------------------------------------------------------------
def contingency(pred, truth, K, C, table=None):
    """-> (table int64 [K, C], skipped)"""
    pred, truth = np.asarray(pred, np.int64).reshape(-1), np.asarray(truth, np.int64).reshape(-1)
    ok = (pred >= 0) & (pred < K) & (truth >= 0) & (truth < C)
    table = np.zeros((K, C), np.int64) if table is None else table.copy()
    np.add.at(table, (pred[ok], truth[ok]), 1)
    return table, int((~ok).sum())


def choose2(v):
    return v * (v - 1) // 2


def scores(table, variant=None):
    """-> Result(nmi, ari, purity, n, tol_nmi, tol_ari, tol_purity) in the finish kernel's order"""
    table = np.asarray(table, np.int64)
    a, b = table.sum(axis=1), table.sum(axis=0)
    n = int(a.sum())
    if n == 0:
        return Result(nmi=np.nan, ari=np.nan, purity=np.nan, n=0.0, tol_nmi=0.0, tol_ari=0.0, tol_purity=0.0)
    dn = float(n)
    mi, sum_abs, arg_err, terms = 0.0, 0.0, 0.0, 0
    for i, j in zip(*np.nonzero(table)):                   # (row-major)
        x = float(table[i, j])
        term = (x / dn) * np.log((dn * x) / (float(a[i]) * float(b[j])))
        mi += term
        sum_abs += abs(term)
        arg_err += (x / dn) * 4 * V
        terms += 1
    ent = []
    for s in (a, b):
        h = 0.0
        for v in s[s > 0]:
            pr = float(v) / dn
            h += -(pr * np.log(pr))
        ent.append(h)
    hp, ht = ent
    hm = (hp + ht) / 2.0
    if variant == "nmi_geometric":
        nmi = 1.0 if hp == 0 and ht == 0 else mi / np.sqrt(hp * ht) if hp * ht > 0 else 0.0
    else:
        nmi = 1.0 if hp == 0 and ht == 0 else mi / hm
    A, B, P = int(choose2(a).sum()), int(choose2(b).sum()), int(choose2(table).sum())
    E = (float(A) * float(B)) / float(choose2(n)) if n > 1 else 0.0
    num, den = float(P) - E, float(A + B) / 2.0 - E
    if variant == "rand_index":
        T = choose2(n)
        ari = 1.0 if T == 0 else (T - A - B + 2 * P) / T
    else:
        ari = 1.0 if den == 0 else num / den
    # both sides round (two libraries' logs): twice the one-sided bounds of the doc string
    err_mi = (5 + terms) * V * sum_abs + arg_err
    err_hm = ((3 + np.count_nonzero(a) + np.count_nonzero(b)) * hm + 1) * V
    tol_nmi = 2 * SAFETY * ((err_mi + abs(nmi) * err_hm) / hm + V * abs(nmi)) if hm > 0 else 0.0
    big = max(float(P), E, float(A + B) / 2.0)
    tol_ari = SAFETY * (6 * V * big * (1 + abs(ari)) / abs(den) + V * abs(ari)) if den != 0 else 0.0
    purity = float(table.max(axis=1).sum()) / dn
    return Result(nmi=nmi, ari=ari, purity=purity, n=dn, tol_nmi=tol_nmi, tol_ari=tol_ari, tol_purity=SAFETY * V)


def check_scores(got, table):
    """got: {nmi, ari, purity, n}.  None or a string."""
    ref = scores(table)
    if ref.n == 0:
        return None if np.isnan(got[:3]).all() and got[3] == 0 else "n = 0: %s" % (got,)
    for name, g, want, tol in (("nmi", got[0], ref.nmi, ref.tol_nmi), ("ari", got[1], ref.ari, ref.tol_ari),
                               ("purity", got[2], ref.purity, ref.tol_purity), ("n", got[3], ref.n, 0.0)):
        if not abs(g - want) <= tol:
            return "%s = %r, expected %r (bound %g)" % (name, g, want, tol)
    return None


# ---- input builders of the GPU tests ------------------------------------------------------------------------------------------------
def unit_patterns(rng, n, D):
    """rows whose fp64 norm is exactly 1 in any order of addition: one entry of +-1, four of +-1/2 or sixteen of +-1/4"""
    out = np.zeros((n, D), np.float32)
    for r in range(n):
        k = [c for c in (1, 4, 16) if c <= D][int(rng.integers(0, len([c for c in (1, 4, 16) if c <= D])))]
        cols = rng.choice(D, k, replace=False)
        out[r, cols] = rng.choice([-1.0, 1.0], k) / np.sqrt(k)
    return out


def exact_case(N, D, K, metric, seed=0):
    """rows and centroids whose fma chains are exact (every partial sum a small dyadic number) -> (X, m).  Euclidean: integers
    in [-3, 3].  Cosine: rows that are a power of two times a unit pattern, so the prepared rows are the patterns themselves,
    and integer centroids.  Centroid K - 1 duplicates centroid 0, and 128 duplicates 127 where K allows: ties across lanes
    and across column tiles go to the lowest index."""
    rng = np.random.default_rng(seed)
    if metric == EUCLIDEAN:
        X = rng.integers(-3, 4, (N, D)).astype(np.float32)
    else:
        X = unit_patterns(rng, N, D) * np.float32(2.0) ** rng.integers(-2, 3, (N, 1)).astype(np.float32)
    m = rng.integers(-3, 4, (K, D)).astype(np.float32)
    m[~m.any(axis=1), 0] = 1
    if K >= 2:
        m[K - 1] = m[0]
    if K >= 129:
        m[128] = m[127]
    return X, m
