"""NumPy fp64 restatement of pn_knn_search / pn_knn_vote (pathnet_amd/csrc/pn_knn.hip) over the explicit [Sq, N] score matrix,
with the derived error bounds, a tolerant checker that leaves no row out, named WRONG implementations and the input builders
of the GPU tests.  Not a test.

The definition (include/pathnet_hip.h).  A row is live when every entry is finite and, for cosine, its fp64 norm is finite and
> 0; a bank row must also pass bank_valid; exclude names one bank index per query that is no candidate.  Score s = <z_q, z_x>
(cosine: unit rows) or <q, x> (dot).  Order: higher fp32 score first, lower index on equal bits.  count = min(k, candidates).

The bounds.  u = 2^-24 is the fp32 unit round-off, first order in u, times SAFETY = 1.5 (contrast_ref's derivation).
 1. cosine.  z^ = fl32(x / norm): |z^_d - z_d| <= u |z_d|, two operands: 2u; the MFMA is one k-ordered fma chain of D products,
    |fl(<z^_q, z^_x>) - <z^_q, z^_x>| <= D u sum_d |z_qd z_xd| <= D u (Cauchy-Schwarz); the restatement's own rounding of the
    returned score to fp32 and slack for the fp64 norms: 2u more.          E = (D + 4) u                   tol_cosine
 2. dot.  The operands are exact; the chain alone:  E_qx = D u sum_d |q_d x_d|  per pair (it also covers the final rounding
    of the true score to fp32, u |s| <= u sum |q_d x_d|).                                               tol_dot
    With integer entries and sum_d |q_d x_d| < 2^24 every partial sum is an integer below 2^24: the chain is EXACT.
 3. vote.  Everything is fp64, v = 2^-53.  w_j = exp(a_j), a_j = (s_j - s_0) / T <= 0: the subtraction of two fp32 values is
    exact in fp64, the division rounds (relative v, an absolute error |a_j| v of the argument = a relative error |a_j| v of
    the exponential), exp is good to 1 ulp (2v): (|a_j| + 3) v.  A class's votes and the total are sums of at most k
    positive terms added one by one: (k - 1) v each, no cancellation.  prob = votes / total, one more rounding:
        |prob^ - prob| <= SAFETY (2 (A + k + 3) + 1) v prob,   A = max_j |a_j| over the voting slots     tol_prob
    T = inf: every weight is 1, the sums are small integers: exact.  The label is decided wherever the two largest class
    votes differ by more than twice that bound of the larger one (vote_margins); exact ties go to the lowest class.
"""
import ctypes
import functools

import numpy as np

U = 2.0 ** -24
V = 2.0 ** -53
SAFETY = 1.5
MAX_K = 64
COSINE, DOT = 0, 1

VARIANTS = ("ties_high", "self", "deadbank", "novalid", "droplast", "droppart", "unsorted", "abs", "nonorm")


class Result:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@functools.lru_cache(maxsize=None)
def plan(Sq, N, D, k, splits=0):
    """{splits, workgroups, row tile, column tile} from the library (needs no GPU)"""
    from pathnet_amd import _lib
    out = (ctypes.c_int64 * 4)()
    _lib.check(_lib.load().pn_knn_plan(Sq, N, D, k, splits, out))
    return tuple(int(v) for v in out)


def workspace_bytes(Sq, N, D, k, splits=0):
    from pathnet_amd import _lib
    need = ctypes.c_int64(-1)
    _lib.check(_lib.load().pn_knn_workspace_bytes(Sq, N, D, k, splits, ctypes.byref(need)))
    return need.value


def rows_ok(X, metric):
    """-> (ok [n] bool, norm [n], the rows the scores are formed from, fp64, dead rows zeroed)"""
    X = np.asarray(X, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        fin = np.isfinite(X).all(axis=1)
        Xz = np.where(fin[:, None], X, 0.0)
        norm = np.sqrt((Xz ** 2).sum(axis=1))
    ok = fin & ((metric == DOT) | (np.isfinite(norm) & (norm > 0)))
    Z = np.where(ok[:, None], Xz, 0.0)
    if metric == COSINE:
        Z = Z / np.where(ok, norm, 1.0)[:, None]
    return ok, norm, Z


def truth(Q, X, metric, bank_valid=None, exclude=None):
    """-> Result(s [Sq, N] fp64 true scores, cand [Sq, N] bool, E [Sq, N] bound per pair, qlive, counts)"""
    Sq, D = np.asarray(Q).shape
    N = np.asarray(X).shape[0]
    qok, _, ZQ = rows_ok(Q, metric)
    xok, _, ZX = rows_ok(X, metric)
    valid = np.ones(N, bool) if bank_valid is None else (np.asarray(bank_valid).reshape(-1) != 0)
    cand = qok[:, None] & (xok & valid)[None, :]
    if exclude is not None:
        e = np.asarray(exclude, np.int64).reshape(-1)
        hit = (e >= 0) & (e < N)
        cand[np.flatnonzero(hit), e[hit]] = False
    s = ZQ @ ZX.T
    if metric == COSINE:
        E = np.full((Sq, N), SAFETY * (D + 4) * U)
    else:
        E = SAFETY * D * U * (np.abs(ZQ) @ np.abs(ZX).T)
    return Result(Sq=Sq, N=N, D=D, metric=metric, s=s, cand=cand, E=E, qlive=qok, ZQ=ZQ, ZX=ZX,
                  counts=np.array([int((~qok).sum()), int((valid & ~xok).sum())], np.int64))


def select(s, cand, k, high_ties=False, key=None):
    """the k best candidates of every row by (fp32 score descending, index ascending) -> (index, score fp32, count)"""
    Sq, N = s.shape
    s32 = s.astype(np.float32) + np.float32(0.0)
    rank = s32 if key is None else key.astype(np.float32)
    index = np.full((Sq, k), -1, np.int64)
    score = np.full((Sq, k), -np.inf, np.float32)
    count = np.zeros(Sq, np.int32)
    cols = np.arange(N)
    for r in range(Sq):
        c = cols[cand[r]]
        order = np.lexsort((-c if high_ties else c, -rank[r, c].astype(np.float64)))[:k]
        n = len(order)
        index[r, :n], score[r, :n], count[r] = c[order], s32[r, c[order]], n
    return index, score, count


def reference(Q, X, k, metric, bank_valid=None, exclude=None, variant=None):
    """The definition.  variant: one of VARIANTS, a named WRONG implementation."""
    t = truth(Q, X, metric, None if variant == "novalid" else bank_valid, None if variant == "self" else exclude)
    s, cand = t.s, t.cand.copy()
    N = t.N
    if variant == "deadbank":          # dead bank rows enter as the zero rows the kernel stores for them
        valid = np.ones(N, bool) if bank_valid is None else (np.asarray(bank_valid).reshape(-1) != 0)
        extra = t.qlive[:, None] & valid[None, :]
        if exclude is not None:
            e = np.asarray(exclude, np.int64).reshape(-1)
            hit = (e >= 0) & (e < N)
            extra[np.flatnonzero(hit), e[hit]] = False
        cand |= extra
    if variant == "droplast":
        cand[:, np.arange(N) % 128 == 127] = False
    if variant == "droppart":
        tiles = -(-N // 128)
        cand[:, 128 * (2 * tiles // 3):] = False
    if variant == "nonorm" and metric == COSINE:
        s = truth(Q, X, DOT).s
    index, score, count = select(s, cand, k, high_ties=variant == "ties_high", key=np.abs(s) if variant == "abs" else None)
    if variant == "unsorted":
        for r in range(t.Sq):
            n = count[r]
            index[r, :n], score[r, :n] = index[r, :n][::-1].copy(), score[r, :n][::-1].copy()
    return Result(index=index, score=score, count=count, counts=t.counts)


def check(got, Q, X, k, metric, bank_valid=None, exclude=None, t=None):
    """The tolerant checker: None when `got` (index, score, count, counts) is an acceptable answer, else a string naming
    the first failure.  Every query row is examined."""
    t = t or truth(Q, X, metric, bank_valid, exclude)
    index, score, count, counts = (np.asarray(getattr(got, f)) for f in ("index", "score", "count", "counts"))
    if index.shape != (t.Sq, k) or score.shape != (t.Sq, k) or count.shape != (t.Sq,):
        return "shapes %s %s %s" % (index.shape, score.shape, count.shape)
    if counts.tolist() != t.counts.tolist():
        return "counts %s, want %s" % (counts.tolist(), t.counts.tolist())
    for r in range(t.Sq):
        c = np.flatnonzero(t.cand[r])
        n = min(k, len(c))
        if count[r] != n:
            return "row %d: count %d, want %d" % (r, count[r], n)
        if (index[r, n:] != -1).any() or not (np.isneginf(score[r, n:])).all():
            return "row %d: slots past count are not -1 / -inf" % r
        idx, sc = index[r, :n], score[r, :n]
        if n == 0:
            continue
        if (idx < 0).any() or (idx >= t.N).any() or not t.cand[r, idx].all():
            return "row %d: an index that is no candidate" % r
        if len(set(idx.tolist())) != n:
            return "row %d: an index twice" % r
        true = t.s[r]
        if not (np.abs(sc.astype(np.float64) - true[idx]) <= t.E[r, idx]).all():
            return "row %d: a score off by %g of its bound" % (r, (np.abs(sc - true[idx]) / np.maximum(t.E[r, idx], 1e-300)).max())
        Erow = t.E[r, c].max()
        kth = np.sort(true[c])[::-1][n - 1]
        if (true[idx] < kth - 2 * Erow).any():
            return "row %d: a neighbour below the k-th true score by more than 2E" % r
        omitted = np.setdiff1d(c, idx)
        if len(omitted) and true[omitted].max() > kth + 2 * Erow:
            return "row %d: an omitted candidate above the k-th true score by more than 2E" % r
        if (np.diff(sc) > 0).any():
            return "row %d: scores increase" % r
        same = sc[1:].view(np.int32) == sc[:-1].view(np.int32)
        if (np.diff(idx)[same] <= 0).any():
            return "row %d: equal score bits without ascending index" % r
    return None


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def make_inputs(kind, Sq, N, D, seed=0):
    """-> (Q, X fp32, bank_valid uint8 [N] or None, exclude int64 [Sq] or None).  Plain normal entries (scores of both signs, so
    that ranking by |s| differs), row norms spread over a factor of ~20 (so that a forgotten normalisation differs)."""
    rng = np.random.default_rng(100000 * Sq + 100 * N + D + 7 * seed)
    X = rng.standard_normal((N, D)) * np.exp(rng.uniform(-1.5, 1.5, (N, 1)))
    Q = rng.standard_normal((Sq, D)) * np.exp(rng.uniform(-1.5, 1.5, (Sq, 1)))
    valid = exclude = None
    if kind == "self":                  # the queries are the first bank rows (or the bank repeated)
        Q = X[np.arange(Sq) % N].copy()
        exclude = (np.arange(Sq) % N).astype(np.int64)
    Q, X = Q.astype(np.float32), X.astype(np.float32)
    pick = lambda n, m: rng.permutation(n)[:max(1, n // m)] if n >= 2 else np.zeros(0, np.int64)        # noqa: E731
    if kind in ("dead", "mix", "deadfew"):
        for A, v in ((X, np.nan), (X, np.inf), (Q, -np.inf), (Q, np.nan)):
            rows = pick(len(A), 9)
            A[rows, rng.integers(0, D, len(rows))] = v
        X[pick(N, 10)] = 0.0            # zero norm: dead for cosine, live for dot
        Q[pick(Sq, 10)] = 0.0
        X[pick(N, 7)] *= np.float32(1e-20)      # squares underflow / overflow in fp32: the norms need fp64
        Q[pick(Sq, 7)] *= np.float32(1e15)
    if kind in ("valid", "mix"):
        valid = (rng.random(N) < 0.7).astype(np.uint8)
        valid[N - 1] = 1
    if kind in ("fewvalid", "deadfew"):
        valid = (rng.random(N) < 0.25).astype(np.uint8)
        valid[0] = 1
    if kind in ("exclude", "mix"):
        exclude = rng.integers(-1, N + 2, Sq).astype(np.int64)      # -1 and N, N + 1: none
        exclude[0] = 0 if N > 1 else -1
    return Q, X, valid, exclude


# (kind, Sq, N, D, k, metric): a covering subset of Sq in {1, 63, 64, 65, 130}, N in {1, 127, 128, 129, 257, 400}, D in {1, 15, 16,
# 17, 33, 128}, k in {1, 2, 5, 32, 64}, with k > N, k > live candidates, both metrics, bank_valid, exclude and dead rows
CASES = (
    ("plain", 1, 1, 1, 1, COSINE),
    ("plain", 63, 127, 15, 2, DOT),
    ("valid", 64, 128, 16, 5, COSINE),
    ("exclude", 65, 129, 17, 32, DOT),
    ("mix", 130, 257, 33, 64, COSINE),
    ("self", 65, 400, 128, 5, COSINE),
    ("plain", 64, 1, 16, 5, DOT),
    ("mix", 1, 400, 33, 64, DOT),
    ("plain", 130, 127, 1, 32, COSINE),
    ("dead", 63, 257, 128, 2, DOT),
    ("deadfew", 65, 129, 15, 64, COSINE),
    ("fewvalid", 64, 128, 17, 64, DOT),
    ("self", 130, 128, 16, 1, DOT),
    ("plain", 65, 400, 15, 32, COSINE),
)


@functools.lru_cache(maxsize=None)
def case(i):
    """-> (Q, X, valid, exclude, k, metric, truth); computed once and shared -- leave the arrays unchanged"""
    kind, Sq, N, D, k, metric = CASES[i]
    Q, X, valid, exclude = make_inputs(kind, Sq, N, D)
    for x in (Q, X, valid, exclude):
        if x is not None:
            x.setflags(write=False)
    return Q, X, valid, exclude, k, metric, truth(Q, X, metric, valid, exclude)


# integer cases of the dot metric: (Sq, N, D, k, lo, hi) entries uniform in [lo, hi]; [-1, 1] at small D ties heavily
INT_CASES = ((65, 257, 17, 32, -8, 8), (64, 400, 128, 64, -8, 8), (130, 129, 3, 64, -1, 1), (1, 128, 1, 5, -8, 8))


@functools.lru_cache(maxsize=None)
def int_case(i):
    """-> (Q, X fp32 with integer entries, k, index, score int64): the exact answer in integer arithmetic"""
    Sq, N, D, k, lo, hi = INT_CASES[i]
    rng = np.random.default_rng(31 + i)
    Q, X = rng.integers(lo, hi + 1, (Sq, D)), rng.integers(lo, hi + 1, (N, D))
    s = Q @ X.T
    index = np.full((Sq, k), -1, np.int64)
    score = np.zeros((Sq, k), np.int64)
    for r in range(Sq):
        order = np.lexsort((np.arange(N), -s[r]))[:k]
        index[r, :len(order)], score[r, :len(order)] = order, s[r, order]
    return Q.astype(np.float32), X.astype(np.float32), k, index, score, int((np.abs(Q) @ np.abs(X).T).max())


# ---- the vote -------------------------------------------------------------------------------------------------------------------
def vote_reference(index, score, count, bank_labels, C, T, labels=None):
    """-> Result(prob fp64 [Sq, C], label int64, confusion, skipped, margin [Sq], tol [Sq, C], exact)"""
    index, score, count = np.asarray(index), np.asarray(score, np.float32), np.asarray(count)
    bank_labels = np.asarray(bank_labels, np.int64)
    Sq, k = index.shape
    N = len(bank_labels)
    prob = np.zeros((Sq, C))
    label = np.full(Sq, -1, np.int64)
    margin = np.full(Sq, np.inf)
    tol = np.zeros((Sq, C))
    for q in range(Sq):
        votes = np.zeros(C)
        total, amax = 0.0, 0.0
        for j in range(min(max(int(count[q]), 0), k)):
            i = index[q, j]
            if not 0 <= i < N or not 0 <= bank_labels[i] < C:
                continue
            diff = 0.0 if score[q, j] == score[q, 0] else float(score[q, j]) - float(score[q, 0])
            with np.errstate(over="ignore", invalid="ignore"):
                w = 1.0 if np.isinf(T) else float(np.exp(np.float64(diff) / T))
            w = w if w >= 0 else 0.0
            amax = max(amax, abs(diff / T) if np.isfinite(diff) and not np.isinf(T) else 0.0)
            votes[bank_labels[i]] += w
            total += w
        if total > 0:
            prob[q] = votes / total
            label[q] = int(np.argmax(votes))
            rel = 0.0 if np.isinf(T) else SAFETY * (2 * (amax + k + 3) + 1) * V
            tol[q] = rel * prob[q] + 1e-300
            top = np.sort(prob[q])[::-1]
            if C > 1 and top[0] != top[1]:
                margin[q] = (top[0] - top[1]) / max(2 * rel * top[0], 1e-300)
            elif C > 1:
                margin[q] = np.inf if np.isinf(T) else 0.0      # an exact tie is decided (lowest class) only in integer sums
    conf = skipped = None
    if labels is not None:
        labels = np.asarray(labels, np.int64)
        conf = np.zeros((C, C), np.int64)
        skipped = np.zeros(1, np.int64)
        for q in range(Sq):
            if 0 <= labels[q] < C and label[q] >= 0:
                conf[labels[q], label[q]] += 1
            else:
                skipped[0] += 1
    return Result(prob=prob, label=label, confusion=conf, skipped=skipped, margin=margin, tol=tol)


# (Sq, k, N, C, T): C in {1, 2, 7, 65}, T = inf with ties, out-of-range labels, count == 0 rows; every row of every case is
# decided (test_knn_ref_host.py asserts it), so labels, confusion and skipped are compared exactly
VOTE_CASES = ((70, 20, 300, 7, 0.07), (33, 64, 100, 2, 0.5), (65, 5, 50, 65, 0.07), (40, 32, 64, 1, 1.0),
              (70, 20, 300, 7, np.inf), (64, 4, 16, 2, np.inf))


@functools.lru_cache(maxsize=None)
def vote_case(i):
    """-> (index, score, count, bank_labels, C, T, labels, reference).  Synthetic neighbour lists: distinct indices, scores
    descending from a cosine-like range, a few -1 indices inside the count, bank labels from -1 to C (both out of range),
    rows with count 0 and count < k."""
    Sq, k, N, C, T = VOTE_CASES[i]
    rng = np.random.default_rng(77 + i)
    index = np.stack([rng.permutation(N)[:k] for _ in range(Sq)]).astype(np.int64)
    score = -np.sort(-rng.uniform(-0.2, 1.0, (Sq, k)), axis=1).astype(np.float32)
    if np.isinf(T):     # quantised: exact ties among the scores, where nothing depends on them.  At a finite T equal scores
        score = (np.round(score * 64) / 64).astype(np.float32)      # would make exact vote ties, which no bound decides
    count = rng.integers(0, k + 1, Sq).astype(np.int32)
    count[0], count[Sq - 1] = 0, k
    index[rng.random((Sq, k)) < 0.03] = -1
    bank_labels = rng.integers(-1, C + 1, N).astype(np.int64)
    bank_labels[0], bank_labels[1] = -1, C
    labels = rng.integers(-1, C + 1, Sq).astype(np.int64)
    labels[0], labels[1] = C, -1
    for j in range(Sq):
        index[j, count[j]:], score[j, count[j]:] = -1, -np.inf
    ref = vote_reference(index, score, count, bank_labels, C, T, labels)
    for x in (index, score, count, bank_labels, labels):
        x.setflags(write=False)
    return index, score, count, bank_labels, C, T, labels, ref
