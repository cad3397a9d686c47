"""CPU restatement of the second-order (return / in-out biased) walk of pn_sample_paths_biased, in NumPy.

The specification (include/pathnet_hip.h, INTEGRATION.md section 2 "Biased walks"), followed literally:

  target of step t >= 1 at node cur, having come from prev:  P(x) ~ P_table(cur -> x) * a(prev, x),
      a = 1/p if x == prev (class 0), 1 if prev -> x is a directed edge of the hop source (class 1), 1/q otherwise (class 2);
      step 0 is the plain table step.
  thresholds  T_c = floor(ldexp(w_c / max(w), 32)),  w = (1/p, 1, 1/q), weight 0 for an infinite parameter.
  trial j of a walk (j = 0, 1, 2, .. across all its steps) reads Philox block j of subsequence
      walk = ((epoch * n + st) * W + wi):  word 0 >> 1 = slot draw (% len), word 1 >> 1 = alias probability draw,
      word 2 = accept draw (taken iff word 2 < T_class), word 3 unused.  Step 0 takes its first proposal.
  a step that comes to its 64th trial takes that proposal whatever the accept draw and counts in `exhausted`.
  L - 1 transitions; nothing is drawn after the last node.  An empty table where a step needs one: the rest of the path
      repeats the node, no further draws, `empty` is set.
  codes = min(hops(st -> x), L - 1) over the directed edges of the hop source.

The alias roll is the reference's:  (1.0 * r1 / RAND_MAX > S[slot]) ? A[slot] : B[slot]  (oracle.merw.alias_build's
tables); uniform tables (pathnet_amd.sampler.build_uniform) have A = B = the neighbour list.
Walks are advanced side by side as arrays; each carries its own step and trial counters, so the order in which walks are
processed has no influence on any of them.
"""
import collections
import math

import numpy as np

MAX_TRIALS = 64
RAND_MAX = 2147483647.0

Result = collections.namedtuple("Result", ("ids", "codes", "exhausted", "empty", "trials", "steps"))


def thresholds(p, q):
    """(T_return, T_near, T_far): Python ints in [0, 2^32]."""
    if not (p > 0 and q > 0):
        raise ValueError("p and q must be > 0")
    w = [0.0 if math.isinf(p) else 1.0 / p, 1.0, 0.0 if math.isinf(q) else 1.0 / q]
    m = max(w)
    return tuple(int(math.floor(math.ldexp(x / m, 32))) for x in w)


def philox_blocks(seed, sub, ctr):
    """Philox4x32-10 (Random123): words [4, N] (uint32) of block ctr[i] of subsequence sub[i] under key `seed`; word k of
    block b is draw 4 b + k of oracle.merw.philox_draw."""
    M = np.uint64(0xFFFFFFFF)
    sub = np.asarray(sub, np.uint64)
    ctr = np.asarray(ctr, np.uint64)
    c0, c1 = ctr & M, ctr >> np.uint64(32)
    c2, c3 = sub & M, sub >> np.uint64(32)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        m0 = np.uint64(0xD2511F53) * c0
        m1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((m1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), m1 & M,
                          (m0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), m0 & M)
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3]).astype(np.uint32)


def merw_tables(n, u, v, p):
    """-> dict(off, A, B, S, eu, ev): the alias tables of the rows (u, v, p) and the hop source's directed edges."""
    from oracle import merw
    off, A, B, S = merw.alias_build(n, u, v, p)
    return dict(n=int(n), off=off, A=A, B=B, S=S, eu=np.asarray(u, np.int64), ev=np.asarray(v, np.int64))


def uniform_tables(n, u, v):
    """-> the same for the uniform sampler's graph (self loop first, then both directions of every pair)."""
    from pathnet_amd import sampler
    off, _, src, nbr = sampler.build_uniform(n, u, v)
    return dict(n=int(n), off=off, A=nbr, B=nbr, S=np.zeros(len(nbr)), eu=src.astype(np.int64), ev=nbr.astype(np.int64))


def hops_from(tb, src, max_hops):
    """{node: hops} of the nodes within max_hops directed hops of src."""
    if "_out" not in tb:
        order = np.argsort(tb["eu"], kind="stable")
        tb["_out"] = (np.searchsorted(tb["eu"][order], np.arange(tb["n"] + 1)), tb["ev"][order])
    o, a = tb["_out"]
    dist = {int(src): 0}
    frontier = [int(src)]
    for h in range(1, max_hops + 1):
        nxt = []
        for x in frontier:
            for y in a[o[x]:o[x + 1]].tolist():
                if y not in dist:
                    dist[y] = h
                    nxt.append(y)
        frontier = nxt
    return dist


def walk(tb, W, L, seed, p, q, sources=None, epoch_begin=0, epoch_count=1, codes=True):
    """-> Result(ids int32 [epoch_count, len(sources), W, L], codes uint8 [...] (or None), exhausted, empty, trials,
    steps): the walks of the listed source nodes (default: every node), trials / steps = all trials and transitions."""
    n, off, A, B, S = tb["n"], tb["off"], tb["A"], tb["B"], tb["S"]
    T = np.array(thresholds(p, q), np.uint64)
    keys = np.unique(tb["eu"] * n + tb["ev"])
    sources = np.arange(n) if sources is None else np.asarray(sources)
    E, Sn = int(epoch_count), len(sources)
    ep = np.repeat(np.arange(epoch_begin, epoch_begin + E, dtype=np.uint64), Sn * W)
    st = np.tile(np.repeat(sources.astype(np.int64), W), E)
    wi = np.tile(np.arange(W, dtype=np.uint64), E * Sn)
    sub = (ep * np.uint64(n) + st.astype(np.uint64)) * np.uint64(W) + wi
    N = len(st)
    ids = np.zeros((N, L), np.int32)
    ids[:, 0] = st
    x, prev = st.copy(), st.copy()
    t = np.zeros(N, np.int64)           # transitions made
    k = np.zeros(N, np.int64)           # trials of the current step
    j = np.zeros(N, np.uint64)          # trials of the walk = the next Philox block
    live = np.full(N, L > 1)
    exhausted = trials = 0
    empty = False
    for _ in range((L - 1) * MAX_TRIALS):
        idx = np.nonzero(live)[0]
        if not len(idx):
            break
        ln = off[x[idx] + 1] - off[x[idx]]
        for i in idx[ln <= 0]:          # an empty table: the rest of the path repeats the node
            ids[i, t[i] + 1:] = x[i]
            live[i] = False
            empty = True
        idx, ln = idx[ln > 0], ln[ln > 0]
        if not len(idx):
            continue
        w = philox_blocks(seed, sub[idx], j[idx])
        j[idx] += np.uint64(1)
        trials += len(idx)
        slot = off[x[idx]] + (w[0] >> 1).astype(np.int64) % ln
        cand = np.where(1.0 * (w[1] >> 1) / RAND_MAX > S[slot], A[slot], B[slot]).astype(np.int64)
        k[idx] += 1
        first = t[idx] == 0
        want = prev[idx] * n + cand
        edge = keys[np.minimum(np.searchsorted(keys, want), len(keys) - 1)] == want
        cls = np.where(cand == prev[idx], 0, np.where(edge, 1, 2))
        capped = ~first & (k[idx] == MAX_TRIALS)
        exhausted += int(capped.sum())
        take = first | (w[2].astype(np.uint64) < T[cls]) | capped
        ti = idx[take]
        prev[ti] = x[ti]
        x[ti] = cand[take]
        t[ti] += 1
        k[ti] = 0
        ids[ti, t[ti]] = x[ti]
        live[ti] = t[ti] < L - 1
    assert not live.any()
    out_codes = None
    if codes and n * n <= 1 << 26:      # the oracle's dense BFS table: 1 + hops, 0 beyond L - 1 hops
        from oracle import merw
        b = merw.bfs_dense(n, tb["eu"].astype(np.int32), tb["ev"].astype(np.int32), L)[st[:, None], ids].astype(np.int64)
        out_codes = np.where(b == 0, L - 1, b - 1).astype(np.uint8)
    elif codes:
        out_codes = np.empty((N, L), np.uint8)
        for s in np.unique(st):
            d = hops_from(tb, s, L - 1)
            rows = np.nonzero(st == s)[0]
            out_codes[rows] = np.vectorize(lambda y: min(d.get(y, L - 1), L - 1), otypes=[np.uint8])(ids[rows])
    shape = (E, Sn, W, L)
    return Result(ids.reshape(shape), None if out_codes is None else out_codes.reshape(shape), exhausted, empty, trials,
                  int(t.sum()))
