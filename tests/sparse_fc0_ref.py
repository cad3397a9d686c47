"""fp64 restatement of fc0 over sparse features, its derived error bound, and the matrices of the edge tests
(tests/test_gpu_sparse_fc0_edges.py runs them on the GPU, tests/test_sparse_fc0_ref_host.py checks this file on the CPU).

The operation (pathnet_amd/csrc/pn_sparse.hip), from the fp32 inputs X [N, F], W [H, F], b [H] and an upstream gradient R [N, H]:
    Xh  = act(X W^T + b)            act = ReLU for PathNet_homo, the identity for PathNet
    g_w = (R * gate)^T X            gate = [Xh > 0] for PathNet_homo, ones for PathNet
    g_b = sum_n (R * gate)[n]
computed here in fp64 (whose own error, ~1e-16 relative, is nine orders below the bound).

The bound, per output ELEMENT, is the forward error of an fp32 sum of k products in any order, with or without FMA
(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: |error| <= gamma_k sum |term|, gamma_k = k u / (1 - k u),
u = 2^-24):
    (k + 4) * 2^-24 * (sum_i |term_i| + |b|)
k: the stored entries of the row (Xh) or of the column (g_w), or N (g_b); + |b| for Xh only.  The + 4 covers the bias add and the
three adds of the weight gradient's four partial sums, and absorbs gamma_k's denominator (k u < 1e-3 at every k used here).  ReLU is
1-Lipschitz, so the bound of the pre-activation holds behind it.  Nothing in it is measured.

The inputs are chosen so that a subtle error is larger than the bound: stored values of X in +-[0.5, 1.5) without row
normalisation, weights of magnitude [0.25, 1] with random signs, R in +-[0.5, 1.5), biases in [-1, 1].  sensitivity() states that
as numbers; the host test holds every value matrix to it:
    delete   leaving one stored entry out of a row's (column's) sum moves EVERY output element of that row (column) by at least
             4 x the element's bound (a dropped term is at least 0.125 (0.25), the bound about 0.04 at 520 entries);
    replace  reading the next stored entry of the same row (column) in an entry's place -- its index and its value -- moves the
             row's (column's) output by at least 4 x the bound in its most affected element, and by that much in more than half
             of its H elements.  (For every element of every pair it cannot hold: two random products differ by less than any
             fixed amount with some probability.  A kernel that misreads an entry fails the comparison as soon as one element
             of the row leaves its bound.)
"""
import functools

import numpy as np

U32 = 2.0 ** -24        # unit roundoff of fp32


def _signed(rng, shape, lo, hi):
    """fp32 values of magnitude [lo, hi) (up to the rounding of the cast) with random signs"""
    return ((lo + (hi - lo) * rng.random(shape)) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


# ---- matrices -------------------------------------------------------------------------------------------------------------------
def from_row_counts(counts, F, rng):
    """X [len(counts), F]: row n holds exactly counts[n] stored entries at random features"""
    X = np.zeros((len(counts), F), np.float32)
    for n, k in enumerate(counts):
        X[n, rng.permutation(F)[:k]] = _signed(rng, k, 0.5, 1.5)
    return X


def from_col_counts(counts, N, rng):
    """X [N, len(counts)]: column f holds exactly counts[f] stored entries at random nodes"""
    return np.ascontiguousarray(from_row_counts(counts, N, rng).T)


def random_matrix(N, F, density, rng):
    return np.where(rng.random((N, F)) < density, _signed(rng, (N, F), 0.5, 1.5), np.float32(0.0)).astype(np.float32)


ROW_STAIR_TAIL = (63, 64, 65, 71, 72, 73, 127, 128, 129, 136)
COL_STAIR_HEAD = (0, 1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 35, 36, 37, 255, 256, 257, 259, 260, 261, 511, 512, 513, 516, 517, 520, 530)
HIDDEN_SIZES = (32, 64, 96, 128, 160, 192, 224, 256, 40, 100)       # 40 and 100: the module pads them to 64 and 128
NODE_COUNTS = (1, 3, 15, 16, 17, 63, 64, 65, 128)


def row_stair_counts():
    """200 rows: n entries in row n for n = 0 .. 136, then 63, 64, 65, 71, 72, 73, 127, 128, 129, 136 over and over"""
    return list(range(137)) + [ROW_STAIR_TAIL[i % len(ROW_STAIR_TAIL)] for i in range(63)]


def col_stair_counts():
    """72 columns: the 28 counts of COL_STAIR_HEAD, then 44 random counts below 64"""
    return list(COL_STAIR_HEAD) + [int(k) for k in np.random.default_rng(72).integers(0, 64, 72 - len(COL_STAIR_HEAD))]


@functools.lru_cache(maxsize=None)
def matrix(name, N=None):
    """the fp32 feature matrix of a value case, computed once and never modified (the array is read-only)"""
    rng = np.random.default_rng([len(name), sum(name.encode()), N or 0])
    if name == "rows":          # N = 200, F = 136
        X = from_row_counts(row_stair_counts(), 136, rng)
    elif name == "cols":        # N = 530, F = 72
        X = from_col_counts(col_stair_counts(), 530, rng)
    elif name == "hidden":      # about 40 % stored
        X = random_matrix(130, 40, 0.4, rng)
    elif name == "nodes":       # F = 9, about half stored, no matrix without an entry
        X = random_matrix(N, 9, 0.5, rng)
        if not X.any():
            X[0, 4] = 0.75
    elif name == "round":       # more rows than one scan round; the rows past 4096 all hold entries
        X = random_matrix(4100, 24, 0.05, rng)
        for n in range(4096, 4100):
            X[n, rng.permutation(24)[:3]] = _signed(rng, 3, 0.5, 1.5)
    elif name == "empty":
        X = np.zeros((67, 13), np.float32)
    elif name == "single":
        X = np.zeros((67, 13), np.float32)
        X[66, 12] = 0.75
    else:
        raise KeyError(name)
    X.setflags(write=False)
    return X


# (matrix name, N or None, module hidden size) of every value case
VALUE_CASES = ([("rows", None, H) for H in (32, 128)] + [("cols", None, H) for H in (32, 128)] +
               [("hidden", None, H) for H in HIDDEN_SIZES] + [("nodes", N, 64) for N in NODE_COUNTS] +
               [("round", None, 32), ("empty", None, 64), ("single", None, 64)])


@functools.lru_cache(maxsize=None)
def operands(name, N, H):
    """(X, W [H, F], b [H], R [N, H]) of a value case, fp32, read-only"""
    X = matrix(name, N)
    rng = np.random.default_rng([7, len(name), sum(name.encode()), N or 0, H])
    W = _signed(rng, (H, X.shape[1]), 0.25, 1.0)
    b = (2.0 * rng.random(H) - 1.0).astype(np.float32)
    R = _signed(rng, (X.shape[0], H), 0.5, 1.5)
    for t in (W, b, R):
        t.setflags(write=False)
    return X, W, b, R


def structure_matrix(N, F, seed=0):
    """about 30 % stored, with some all-zero rows and columns where the shape has room for them; 1 x 1: its entry is stored"""
    rng = np.random.default_rng([11, N, F, seed])
    X = random_matrix(N, F, 0.3, rng)
    if N >= 4:
        X[rng.permutation(N)[:max(1, N // 16)], :] = 0.0
    if F >= 4:
        X[:, rng.permutation(F)[:max(1, F // 16)]] = 0.0
    if N * F == 1:
        X[0, 0] = -1.25
    return X


def carry_matrix():
    """4097 x 900: row 4096 -- the only count of the scan's second round -- is full (900 entries) and the 4096 rows in front of
    it hold 600 between them, so most entries lie behind the round boundary and a lost carry is 600, not an off-by-few"""
    rng = np.random.default_rng(4097)
    X = np.zeros((4097, 900), np.float32)
    at = rng.permutation(4096 * 900)[:600]
    X[at // 900, at % 900] = _signed(rng, 600, 0.5, 1.5)
    X[4096, :] = _signed(rng, 900, 0.5, 1.5)
    return X


# ---- reference and bound ----------------------------------------------------------------------------------------------------------
def reference(X, W, b, R, relu, gate=None):
    """fp64 results and per-element bounds.  gate (bool [N, H], or None: ones) multiplies R in the two gradients."""
    X64, W64, b64 = X.astype(np.float64), W.astype(np.float64), b.astype(np.float64)
    G = R.astype(np.float64) if gate is None else R.astype(np.float64) * gate
    stored = X != 0
    k_row, k_col = stored.sum(1), stored.sum(0)
    pre = X64 @ W64.T + b64
    out = dict(pre=pre, Xh=np.maximum(pre, 0.0) if relu else pre, g_w=G.T @ X64, g_b=G.sum(0))
    out["bound_Xh"] = (k_row[:, None] + 4) * U32 * (np.abs(X64) @ np.abs(W64).T + np.abs(b64))
    out["bound_g_w"] = (k_col[None, :] + 4) * U32 * (np.abs(G).T @ np.abs(X64))
    out["bound_g_b"] = (X.shape[0] + 4) * U32 * np.abs(G).sum(0)
    return out


def ratio(got, want, bound):
    """|got - want| / bound, element by element: 0 where both are 0, inf where an error meets a zero bound"""
    err = np.abs(np.asarray(got, np.float64) - want)
    out = np.zeros_like(err)
    np.divide(err, bound, out=out, where=bound > 0)
    out[(bound == 0) & (err > 0)] = np.inf
    out[~np.isfinite(err)] = np.inf
    return out


def sensitivity(X, W, b, R):
    """How far above the bound a one-entry mistake lands, on the ungated formulas (see the module's docstring):
    {"delete_Xh", "replace_Xh", "delete_g_w", "replace_g_w"} -> the smallest ratio change / bound (inf: nothing to get wrong);
    {"share_Xh", "share_g_w"} -> the smallest share, over the neighbour pairs, of a line's H elements a replacement moves by at
    least 4 x their bound (1.0: no pair)."""
    ref = reference(X, W, b, R, relu=False)
    out = {}
    for key, (r, c), other, bound in (("Xh", np.nonzero(X), W.astype(np.float64).T, ref["bound_Xh"]),
                                      ("g_w", np.nonzero(X.T)[::-1], R.astype(np.float64), ref["bound_g_w"].T)):
        if key == "Xh":         # entries in row-major order; entry (n, f) adds x * W[:, f] to Xh[n, :]
            T, B, line = X[r, c].astype(np.float64)[:, None] * other[c], bound[r], r
        else:                   # entries in column-major order; entry (n, f) adds x * R[n, :] to g_w[:, f]
            T, B, line = X[r, c].astype(np.float64)[:, None] * other[r], bound[c], c
        out["delete_" + key] = float((np.abs(T) / B).min()) if len(T) else np.inf
        same = line[1:] == line[:-1]
        moved = (np.abs(T[1:] - T[:-1]) / B[1:])[same]
        out["replace_" + key] = float(moved.max(1).min()) if len(moved) else np.inf
        out["share_" + key] = float((moved >= 4.0).mean(1).min()) if len(moved) else 1.0
    return out
