"""Test-side restatements of the path-pattern census (no package code): the level-by-level recurrence
    C_0[v] = [1],   C_j[u][b * B^(j-1) + r] = sum over the entries v of u's list with s[v] == b of C_(j-1)[v][r]
over the undirected multiset lists of the rows -- every row (u, v) puts v into u's list and u into v's, repeats kept,
a row u == u adds two entries -- once in plain NumPy and once with scipy.sparse for the large graphs."""
import numpy as np


def entries(u, v):
    """-> (owner, entry) int64 [2m]: both directions of every row."""
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    return np.concatenate([u, v]), np.concatenate([v, u])


def default_symbols(n):
    return (np.arange(n) & 1).astype(np.int64)


def counts_numpy(n, u, v, k, symbols=None, B=2):
    own, ent = entries(u, v)
    s = default_symbols(n) if symbols is None else np.asarray(symbols, np.int64)
    C = np.ones((n, 1), np.int64)
    for _ in range(k):
        R = C.shape[1]
        nxt = np.zeros((n, B * R), np.int64)
        for r in range(R):
            np.add.at(nxt, (own, s[ent] * R + r), C[ent, r])
        C = nxt
    return C


def counts_sparse(n, u, v, k, symbols=None, B=2):
    import scipy.sparse as sp
    own, ent = entries(u, v)
    s = default_symbols(n) if symbols is None else np.asarray(symbols, np.int64)
    mats = []
    for b in range(B):
        pick = s[ent] == b
        mats.append(sp.csr_matrix((np.ones(int(pick.sum()), np.int64), (own[pick], ent[pick])), shape=(n, n)))
    C = np.ones((n, 1), np.int64)
    for _ in range(k):
        C = np.concatenate([np.asarray(A @ C) for A in mats], axis=1)       # block b holds the patterns b * R + r
    assert C.dtype == np.int64
    return C


def labels_of(counts):
    """Lowest index among the largest counts (np.argmax returns the first)."""
    return np.argmax(counts, axis=1).astype(np.int64)
