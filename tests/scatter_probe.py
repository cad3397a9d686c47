"""Probe parameters, paths and an integer reference that hold the backward's scatter-adds to EXACT counts.
Shared by tests/test_scatter_probe_host.py, which proves every construction on the CPU oracle alone, and
tests/test_gpu_scatter_exact.py, which runs the same cases through the library's four scatter routes (fp32 atomics, the
sorted two-pass det_scatter_kernel of pn_det.hip, either over compact rows, either per micro-batch).

The construction is that of tests/dropout_probes.py for the sum / mean encoders: F = H, X = 0, fc0 = (I, 1), the distance
layer of code c at (0.5 amp[c] I, 0.5 amp[c]) with amp[c] = 2^c, fc2 = 1 / C, and optionally attw.weight[0, H:] = 2^-m.
Every projected row is 1, every table row (node, c) is 2^c in every column, and under the upstream gradient
G[s] = (C g_s, 0, ...) with small integers g_s every quantity of the backward is a dyadic rational with a few significant
bits: every fp32 sum is exact IN ANY ORDER (reference() returns the bound that proves it per case), every column of a row is
equal, and

    X.grad[n] = sum over the path steps (q, t) on node n of 0.5 amp[code] * d y[q]  +  sum over s with sel[s] = n of g_s
                (+ the attention-ego term: homo through the table row of (q, 0), hetero onto the row of ids[q, 0]),

    d y[q] = g[group(q)] * k / Lk,   k = 1 / W (PAGG), (1 + att_q) / W (homo), 1 / W^2 (hetero),   Lk = L (mean) or 1 (sum).

reference() computes that -- and the bank's, fc0.bias's and the attention weights' gradients -- with numpy int64 numerators
over one power-of-two denominator per tensor and np.add.at over the index plan: neither the oracle nor the library.

The paths come from a run-length specification (build_paths): the stably sorted key sequence of ONE of the backward's three
scatters -- DET_ROW (keys node * L + code of every path step), DET_SEL (keys sel), DET_EGO (keys: homo the table row of
step 0, hetero ids[q, 0]) -- has exactly the given runs of equal keys in the given order, per micro-batch, so that a case
sits on a chosen edge of det_scatter_kernel: chunks of DET_CHUNK sorted positions, runs that cross them, 256 / (H / 4) lane
groups per workgroup, two scatters in one launch.  chunk_classes names the edges a key sequence contains."""
import os
import re

import numpy as np
import torch

import dropout_probes as dp
from conftest import ROOT
from oracle import pagg_oracle as po
from test_gpu_compact_rows import plan_to_paths


def read_det_chunk():
    txt = open(os.path.join(ROOT, "pathnet_amd", "csrc", "pn_det.h")).read()
    m = re.search(r"constexpr\s+int\s+DET_CHUNK\s*=\s*(\d+)\s*;", txt)
    assert m, "pn_det.h no longer defines DET_CHUNK"
    return int(m.group(1))


DET_CHUNK = read_det_chunk()
TABLES_CUT_FOR = 32         # the run-length tables below are cut for this chunk size: revisit them when DET_CHUNK changes
NFILL = 24                  # nodes the steps outside the specified scatter are drawn from


# ---- edge classes of a sorted key sequence --------------------------------------------------------------------------------
K_SIZES = ("K = 1", "K = chunk - 1", "K = chunk", "K = chunk + 1", "K a multiple of chunk, >= 3 chunks",
           "K = 1 mod chunk, >= 3 chunks")
RUN_EDGES = ("all keys distinct", "one run over all K >= 3 chunks + 1 (head, whole middle chunks, ragged tail)",
             "chunk boundary that nothing crosses", "trail piece of one position", "lead piece of one position",
             "lead piece, interior runs and another run's trail piece in one chunk",
             "run starting at a chunk's first position, b > 0, and crossing on", "run filling exactly two aligned chunks",
             "crossing run ending in the ragged last chunk")
SEQUENCE_CLASSES = K_SIZES + RUN_EDGES


def chunk_classes(keys, K, chunk=DET_CHUNK):
    """the edge classes (names of SEQUENCE_CLASSES) that the stably sorted sequence of one scatter's K keys contains"""
    k = np.sort(np.asarray(keys).reshape(-1), kind="stable")
    assert len(k) == K and K >= 1
    nch = -(-K // chunk)
    out = set()
    for name, val in zip(K_SIZES[:4], (1, chunk - 1, chunk, chunk + 1)):
        if K == val:
            out.add(name)
    if K % chunk == 0 and nch >= 3:
        out.add(K_SIZES[4])
    if K % chunk == 1 and nch >= 3:
        out.add(K_SIZES[5])
    starts = np.flatnonzero(np.r_[True, k[1:] != k[:-1]])
    ends = np.r_[starts[1:], K]
    if len(starts) == K and K > 1:
        out.add(RUN_EDGES[0])
    if len(starts) == 1 and K >= 3 * chunk + 1 and K % chunk != 0:
        out.add(RUN_EDGES[1])
    run_of = np.repeat(np.arange(len(starts)), ends - starts)
    for b in range(chunk, K, chunk):
        if k[b - 1] != k[b]:
            out.add(RUN_EDGES[2])
            continue
        s, e = starts[run_of[b]], ends[run_of[b]]
        if s == b - 1:
            out.add(RUN_EDGES[3])
        if e == b + 1:
            out.add(RUN_EDGES[4])
    for c in range(nch):
        b, e = c * chunk, min(K, (c + 1) * chunk)
        lead = b > 0 and k[b - 1] == k[b]
        cont = e < K and k[e] == k[e - 1]
        nruns = run_of[e - 1] - run_of[b] + 1
        if lead and cont and nruns >= 3:
            out.add(RUN_EDGES[5])
        if b > 0 and not lead and cont and nruns == 1:
            out.add(RUN_EDGES[6])
        if e == K and K % chunk != 0 and lead and nruns == 1:
            out.add(RUN_EDGES[8])
    if np.any((starts % chunk == 0) & (ends - starts == 2 * chunk)):
        out.add(RUN_EDGES[7])
    return out


def lane_classes(K, H, chunk=DET_CHUNK):
    """how the chunks of K positions fall onto det_scatter_kernel's workgroups: H / 4 lanes walk a chunk, 256 / (H / 4)
    such groups share a workgroup (H = 96: ten groups and 16 idle threads; H > 512: one chunk per workgroup)"""
    gpb, nch = 256 // (H // 4), -(-K // chunk)
    out = set()
    if gpb > 1 and nch > gpb and nch % gpb:
        out.add("H = %d: more chunks than a workgroup's %d lane groups, no multiple of them" % (H, gpb))
    if gpb == 1 and nch >= 2:
        out.add("a workgroup walks one chunk (H > 512)")
    return out


LANE_CLASSES = ("H = 32: more chunks than a workgroup's 32 lane groups, no multiple of them",
                "H = 96: more chunks than a workgroup's 10 lane groups, no multiple of them",
                "a workgroup walks one chunk (H > 512)")
PAIR_CLASSES = ("homo: DET_SEL and DET_EGO in one launch, K_sel < K_ego", "hetero: DET_SEL, then DET_EGO onto the same d Xh",
                "pagg: no DET_EGO")


# ---- the cases ------------------------------------------------------------------------------------------------------------
# run-length lists (sorted positions; | marks the chunk boundaries at 32, 64, ...)
#   EDGES, K = 160 = 5 chunks: 0..30 | 31..32 (trail piece = position 31 alone, lead piece = position 32 alone) |
#   two interior runs 33..42, then 43..70 (chunk 1 holds a lead piece, interior runs and another run's trail piece) |
#   71..95 ends on chunk 2's last position, a new key opens chunk 3 (nothing crosses) | 96..159 starts at a chunk's first
#   position, b > 0, crosses on and fills exactly two aligned chunks
EDGES = [31, 2, 5, 5, 28, 25, 64]
ONE_RUN_97 = [97]                   # K = 1 mod 32, four chunks: head at 0, two whole middle chunks, a one-position ragged tail
DISTINCT_33 = [1] * 33              # K = 33: all keys distinct, a second chunk of one position
TWO_31 = [10, 21]                   # K = 31: one ragged chunk
TWO_32 = [16, 16]                   # K = 32: one full chunk, e == K
ONE_1 = [1]                         # K = 1
TAIL_100 = [97, 3]                  # a crossing run that ends inside the ragged last chunk, then one more run


class Case:
    """id, class, encoder, H, W, L, C, att (None: attw = 0, else m: attw.weight[0, H:] = 2^-m), the scatter whose runs are
    specified ("row" / "sel" / "ego"), its run lengths per micro-batch (one list: the library's own micro-batches are cut
    from it), ego_first (column 0 of every path is its masked node), and what the line is there for"""

    def __init__(self, cid, variant, cell, H, W, L, C, att, target, parts, ego_first, why):
        self.id, self.variant, self.cell, self.H, self.W, self.L, self.C = cid, variant, cell, H, W, L, C
        self.att, self.target, self.parts, self.ego_first, self.why = att, target, parts, ego_first, why
        assert cell in ("sum", "mean") and (cell == "sum" or L & (L - 1) == 0) and W & (W - 1) == 0 and C & (C - 1) == 0
        self._data = None

    @property
    def data(self):
        if self._data is None:
            self._data = build_case(self)
        return self._data


def _c(*a):
    return Case(*a)


CASES = [
    # -- one sequence on all three scatters: W = L = 1 and column 0 the masked node make rowidx = egoidx = sel -------------
    _c("homo-edges", "homo", "sum", 128, 1, 1, 4, None, "sel", [EDGES], True, "every crossing / boundary class, 5 chunks"),
    _c("hetero-edges", "hetero", "mean", 256, 1, 1, 2, 8, "sel", [EDGES], True, "the same onto d Xh twice (SEL, then EGO)"),
    _c("pagg-edges", "pagg", "sum", 128, 1, 4, 4, None, "sel", [EDGES], False, "DET_SEL at every edge without DET_EGO (PAGG: L = 4)"),
    _c("homo-one-run-97", "homo", "mean", 32, 1, 1, 8, 8, "sel", [ONE_RUN_97], True, "one run, K = 97: head, middles, tail"),
    _c("hetero-one-run-97", "hetero", "sum", 96, 1, 1, 4, None, "sel", [ONE_RUN_97], True, "one run, K = 97, ten lane groups"),
    _c("pagg-one-run-97", "pagg", "mean", 32, 1, 4, 4, None, "sel", [ONE_RUN_97], False, "one masked node 97 times"),
    _c("homo-distinct-33", "homo", "sum", 288, 1, 1, 4, 8, "sel", [DISTINCT_33], True, "K = 33, all keys distinct, H = 288"),
    _c("hetero-distinct-33", "hetero", "sum", 128, 1, 1, 4, None, "sel", [DISTINCT_33], True, "K = 33, all keys distinct"),
    _c("homo-31", "homo", "sum", 96, 1, 1, 4, None, "sel", [TWO_31], True, "K = 31"),
    _c("hetero-31", "hetero", "mean", 32, 1, 1, 4, 8, "sel", [TWO_31], True, "K = 31"),
    _c("homo-32", "homo", "mean", 256, 1, 1, 4, None, "sel", [TWO_32], True, "K = 32"),
    _c("hetero-32", "hetero", "sum", 288, 1, 1, 2, 8, "sel", [TWO_32], True, "K = 32, H = 288"),
    _c("homo-1", "homo", "sum", 128, 1, 1, 4, 8, "sel", [ONE_1], True, "K = 1"),
    _c("hetero-1", "hetero", "sum", 96, 1, 1, 4, None, "sel", [ONE_1], True, "K = 1"),
    # -- lane groups of a workgroup (DET_ROW) -----------------------------------------------------------------------------
    _c("homo-H32-36-chunks", "homo", "sum", 32, 32, 4, 4, None, "row", [[37] * 31 + [5]], False,
       "K = 1152 > 1024 at H = 32: 36 chunks on 32 lane groups, a second workgroup of four"),
    _c("pagg-H96-12-chunks", "pagg", "mean", 96, 8, 4, 4, None, "row", [[50] * 7 + [34]], False,
       "K = 384 at H = 96: 12 chunks on 10 lane groups"),
    _c("hetero-H1024", "hetero", "sum", 1024, 4, 2, 4, 10, "row", [[20, 13, 7]], False, "H = 1024: a workgroup walks one chunk"),
    _c("homo-H1024", "homo", "mean", 1024, 4, 4, 2, 10, "row", [[33, 31, 48]], False, "H = 1024, four chunks, homo attention"),
    # -- the pooling backward's two scatters with W > 1 -------------------------------------------------------------------
    _c("homo-ego-edges", "homo", "sum", 256, 4, 2, 4, 8, "ego", [EDGES], False, "DET_EGO onto d Z at every edge, K_sel = 40 < K_ego"),
    _c("hetero-ego-edges", "hetero", "mean", 128, 4, 4, 4, 7, "ego", [EDGES], False, "DET_EGO onto d Xh at every edge, behind DET_SEL"),
    _c("homo-shared-ego", "homo", "sum", 128, 8, 2, 4, 8, "sel", [[1] * 20 + [13]], True,
       "repeated masked nodes, step 0 the masked node: the plan's shared ego rows, DET_EGO runs of 8 and 104"),
    _c("pagg-sel-one-run", "pagg", "sum", 288, 2, 4, 4, None, "sel", [ONE_RUN_97], False, "one masked node 97 times, H = 288, W = 2"),
    # -- micro-batches by construction: chunks restart in each --------------------------------------------------------------
    _c("homo-micro-edges", "homo", "sum", 128, 1, 1, 4, None, "sel", [EDGES, EDGES, ONE_RUN_97], True,
       "micro-batches of 160 / 160 / 97 masked nodes, each at its own edges, the same rows in all three"),
    _c("hetero-micro-row", "hetero", "sum", 96, 2, 2, 4, None, "row", [EDGES, EDGES, TAIL_100], False,
       "micro-batches of 40 / 40 / 25 masked nodes: DET_ROW of 160 / 160 / 100 positions"),
]
CASE_IDS = [c.id for c in CASES]


def amp_len(case):
    return 4 if case.variant == "pagg" else case.L          # (PAGG keeps its four distance layers at any walk length)


def probe_params(case):
    """reference state_dict keys -> fp32 tensors"""
    Lb = amp_len(case)
    sd = dp.params(case.variant, case.cell, case.H, Lb, case.C, dp.amp_powers(Lb))
    if case.att is not None:
        assert case.variant != "pagg"
        sd["attw.weight"][0, case.H:] = 2.0 ** -case.att
    return sd


def upstream(S, C):
    """(g [S] int64, G [S, C] fp32): G[s] = (C g_s, 0, ...), g_s = s + 1"""
    g = np.arange(1, S + 1, dtype=np.int64)
    G = torch.zeros(S, C)
    G[:, 0] = torch.as_tensor((C * g).astype(np.float32))
    return g, G


def group_of(variant, S, W):
    return dp.group_of(variant, S, W)


def auto_micro(S):
    """micro-batch size (masked nodes) that cuts S into three micro-batches, the last smaller; 0: S is too small"""
    sb = (S - 1) // 2
    return sb if S >= 5 and S - 2 * sb < sb else 0


# ---- paths from a run-length specification --------------------------------------------------------------------------------
def build_paths(variant, W, L, target, parts, zero_first, ego_first=False, seed=0):
    """-> dict(sel [S], ids [S, W, L], codes [S, W, L], N, sizes: masked nodes per part, pool: the node of run i).
    parts[b]: run lengths of the target scatter's sorted keys over the masked nodes (pooling groups) of part b; run i of
    every part has the same key, node pool[i] = 2 i + 1 (code 0 for "sel" / "ego"; for "row" the codes rise with the runs,
    and with zero_first every step 0 has code 0).  Everything else is filler: steps on NFILL nodes above the pool at random
    codes, distinct masked nodes above those.  Every touched node is odd, every even row of X.grad is untouched."""
    rng = np.random.default_rng(seed)
    per = {"row": W * L, "sel": 1, "ego": W}[target]
    sizes = []
    for runs in parts:
        assert sum(runs) % per == 0, (target, sum(runs), per)
        sizes.append(sum(runs) // per)
    assert len(parts) == 1 or (len(parts) >= 3 and len(set(sizes[:-1])) == 1 and sizes[-1] < sizes[0]), sizes
    S = sum(sizes)
    P = S * W
    bounds = np.r_[0, np.cumsum(sizes)]
    pool = 1 + 2 * np.arange(max(len(r) for r in parts))
    fill = pool[-1] + 2 + 2 * np.arange(NFILL)
    group = group_of(variant, S, W)
    node = fill[rng.integers(0, NFILL, (P, L))]
    code = rng.integers(0, L, (P, L))
    if zero_first:
        code[:, 0] = 0
    if target == "row":
        for b, runs in enumerate(parts):
            Q = np.flatnonzero((group >= bounds[b]) & (group < bounds[b + 1]))
            n = len(Q) * L
            starts = np.r_[0, np.cumsum(runs)[:-1]]
            kn = np.repeat(pool[:len(runs)], runs)
            kc = np.repeat(np.minimum(L - 1, starts * L // n), runs)
            if zero_first:      # the runs that start below n / L have code 0 and cover the len(Q) step-0 positions
                zero = rng.permutation(np.flatnonzero(kc == 0))
                first, rest = zero[:len(Q)], rng.permutation(np.r_[zero[len(Q):], np.flatnonzero(kc != 0)])
                node[Q, 0], code[Q, 0] = kn[first], 0
                node[Q, 1:], code[Q, 1:] = kn[rest].reshape(len(Q), L - 1), kc[rest].reshape(len(Q), L - 1)
            else:
                perm = rng.permutation(n)
                node[Q], code[Q] = kn[perm].reshape(len(Q), L), kc[perm].reshape(len(Q), L)
    ids, codes = plan_to_paths(variant, node, code, S, W, L)
    ids2, codes2 = ids.reshape(P, L), codes.reshape(P, L)       # (views: flat path p = s W + w, the sequence slot q)
    if target == "sel":
        sel = np.concatenate([rng.permutation(np.repeat(pool[:len(r)], r)) for r in parts])
        if ego_first:
            ids2[:, 0], codes2[:, 0] = np.repeat(sel, W), 0
    else:
        assert not ego_first
        sel = rng.permutation(fill[-1] + 2 + 2 * np.arange(S))
    if target == "ego":
        for b, runs in enumerate(parts):
            Q = np.flatnonzero((group >= bounds[b]) & (group < bounds[b + 1]))
            ids2[Q, 0], codes2[Q, 0] = rng.permutation(np.repeat(pool[:len(runs)], runs)), 0
    N = int(max(sel.max(), ids.max())) + 2
    out = dict(sel=sel.astype(np.int64), ids=ids.astype(np.int64), codes=codes.astype(np.int64), N=N, S=S, sizes=sizes, pool=pool)
    for b, runs in enumerate(parts):        # the construction gives the runs it was asked for
        keys = scatter_keys(variant, out["sel"], out["ids"], out["codes"], W, L, (bounds[b], bounds[b + 1]))[target]
        assert run_lengths(keys) == list(runs), (target, b, run_lengths(keys), runs)
    return out


def run_lengths(keys):
    k = np.sort(np.asarray(keys).reshape(-1), kind="stable")
    starts = np.flatnonzero(np.r_[True, k[1:] != k[:-1]])
    return list(np.diff(np.r_[starts, len(k)]))


def scatter_keys(variant, sel, ids, codes, W, L, groups=None):
    """{"row", "sel", "ego"}: the three scatters' keys for the masked nodes [g0, g1) (a micro-batch; default: the batch)
    over the dense table -- rowidx = node * L + code, sel, egoidx (pn_plan.hip: plan_kernel); "ego" is None for PAGG"""
    S = len(sel)
    node, code, group, member, ego = po.plan(variant, ids, codes, S, W, L)
    g0, g1 = groups if groups is not None else (0, S)
    Q = np.flatnonzero((group >= g0) & (group < g1))
    row = node * L + code
    egok = None if variant == "pagg" else ego[Q] if variant == "hetero" else row[Q, 0]
    return {"row": row[Q].reshape(-1), "sel": np.asarray(sel)[g0:g1], "ego": egok}


def build_case(case):
    d = build_paths(case.variant, case.W, case.L, case.target, case.parts, case.att is not None, case.ego_first,
                    seed=CASE_IDS.index(case.id))
    assert d["N"] <= 400 and d["S"] * case.W * case.L <= 1500, (case.id, d["N"], d["S"] * case.W * case.L)
    d["micro"] = d["sizes"][0] if len(case.parts) > 1 else auto_micro(d["S"])
    d["g"], d["G"] = upstream(d["S"], case.C)
    return d


def micro_groups(S, micro):
    """[(g0, g1)] of the micro-batches of `micro` masked nodes"""
    return [(b, min(S, b + micro)) for b in range(0, S, micro)]


def case_classes(case):
    """{"row", "row-micro", "sel", "ego-homo", "ego-hetero", "case"} -> edge classes this case's key sequences contain: the
    whole batch's, the micro-batches' (DET_ROW restarts its chunks in each), and the launch-level ones"""
    d = case.data
    S, W, L = d["S"], case.W, case.L
    out = {k: set() for k in ("row", "row-micro", "sel", "ego-homo", "ego-hetero", "case")}
    spans = [("", (0, S))] + ([("-micro", g) for g in micro_groups(S, d["micro"])] if d["micro"] else [])
    for tag, g in spans:
        keys = scatter_keys(case.variant, d["sel"], d["ids"], d["codes"], W, L, g)
        out["row" + tag] |= chunk_classes(keys["row"], len(keys["row"])) | lane_classes(len(keys["row"]), case.H)
        out["sel"] |= chunk_classes(keys["sel"], len(keys["sel"]))
        if keys["ego"] is not None:
            out["ego-" + case.variant] |= chunk_classes(keys["ego"], len(keys["ego"]))
    if case.variant == "homo" and S < S * W:
        out["case"].add(PAIR_CLASSES[0])
    if case.variant == "hetero":
        out["case"].add(PAIR_CLASSES[1])
    if case.variant == "pagg":
        out["case"].add(PAIR_CLASSES[2])
    return out


# ---- the reference: integer arithmetic alone ------------------------------------------------------------------------------
def _pow2_part(arrays):
    """largest power of two dividing every non-zero entry"""
    v = np.concatenate([np.abs(np.asarray(a, dtype=np.int64)).reshape(-1) for a in arrays])
    v = v[v != 0]
    if not len(v):
        return 1
    g = int(np.gcd.reduce(v))
    return g & -g


def _exact_f32(num, den, shape):
    """num / den (int64 scalar or array, den a power of two) -> fp32 tensor of `shape`, every step checked to be exact"""
    num = np.asarray(num, dtype=np.int64)
    assert np.abs(num).max(initial=0) < 2 ** 53 and den & (den - 1) == 0
    f64 = num.astype(np.float64) / float(den)
    f32 = f64.astype(np.float32)
    assert np.array_equal(f32.astype(np.float64), f64), "the reference does not fit fp32"
    return torch.from_numpy(np.broadcast_to(f32, shape).copy())


def reference(case, drop=None, move=None):
    """-> (want {name: fp32 tensor}, bounds {name: (scale, largest sum of |numerators| of one element)}, touched [N] bool).
    want: X [N, H], the distance layers' weight / bias, fc0.bias and -- with attention -- attw.weight / attw.bias.
    bounds: per tensor (and for the intermediate d Z) every contribution is an integer multiple of `scale`; the second entry
    is the largest sum of |contribution| / scale over one destination element: below 2^24, every
    partial sum of every order is an fp32 integer multiple of `scale`.
    drop / move = (q, t): mutations for the checker's own test -- that path step's contribution to d Z is left out / lands
    on the next node's row."""
    d = case.data
    variant, H, W, L, S = case.variant, case.H, case.W, case.L, d["S"]
    N, P = d["N"], S * W
    node, code, group, member, ego = po.plan(variant, d["ids"], d["codes"], S, W, L)
    Lk = L if case.cell == "mean" else 1
    has, m = case.att is not None, case.att or 0
    A = np.int64(1) << code                     # amp of every step
    hs = A.sum(axis=1)                          # h[q] = hs[q] / Lk in every column
    gq = d["g"][group]
    wgt = np.ones((P, L), np.int64)
    node = node.copy()
    if drop is not None:
        wgt[drop] = 0
    if move is not None:
        node[move] += 1
    # d Z [N, L]: numerators over Dz
    if variant == "homo":
        Dz = W * Lk << m
        sn = gq * ((1 << m) + (H * A[:, 0] if has else 0))         # g (1 + att_q) / (W Lk),  att_q = 2^-m H amp[code(q, 0)]
        en = H * hs * gq if has else None                          # d att_q 2^-m = H h[q] g / W 2^-m onto row (q, 0)
    else:
        Dz = (W * W if variant == "hetero" else W) * Lk
        sn, en = gq, None
    step = sn[:, None] * wgt
    nZ, aZ = np.zeros((N, L), np.int64), np.zeros((N, L), np.int64)
    np.add.at(nZ, (node, code), step)
    np.add.at(aZ, (node, code), np.abs(step))
    if en is not None:
        np.add.at(nZ, (node[:, 0], code[:, 0]), en)
        np.add.at(aZ, (node[:, 0], code[:, 0]), np.abs(en))
    # d Xh = X.grad [N]: numerators over Dx
    dsn = None
    if variant == "hetero":
        tot = np.zeros(S, np.int64)
        np.add.at(tot, group, hs)
        dsn = H * gq * (W * hs - tot[group])       # d score[q] = dsn / (W^3 Lk): softmax backward of uniform weights 1 / W
    ego_on = variant == "hetero" and has
    Dx = 2 * Dz * ((W << m) if ego_on else 1)
    fz = Dx // (2 * Dz)
    amp = (np.int64(1) << np.arange(L))[None, :]
    nX, aX = (nZ * amp).sum(1) * fz, (aZ * amp).sum(1) * fz
    np.add.at(nX, d["sel"], Dx * d["g"])
    np.add.at(aX, d["sel"], Dx * d["g"])
    if ego_on:                                      # d score[q] 2^-m onto the row of ids[q, 0]
        np.add.at(nX, ego, 2 * dsn)
        np.add.at(aX, ego, 2 * np.abs(dsn))
    want, bounds = {}, {}

    def put(name, num, den, shape, contribs, abssum):
        want[name] = _exact_f32(num, den, shape)
        p2 = _pow2_part(contribs)
        bounds[name] = (p2 / den, int(np.max(abssum, initial=0)) // p2)
    x_contribs = [step * amp[0][code] * fz, Dx * d["g"]] + ([2 * dsn] if ego_on else []) + ([en * A[:, 0] * fz] if en is not None else [])
    put("X", nX[:, None], Dx, (N, H), x_contribs, aX)
    bounds["d Z"] = ((_pow2_part([step] + ([en] if en is not None else []))) / Dz,
                     int(aZ.max()) // _pow2_part([step] + ([en] if en is not None else [])))
    put("fc0.bias", nX.sum(), Dx, (H,), x_contribs, aX.sum())
    for c in range(amp_len(case)):
        name = ("nei%d" % c) if variant == "pagg" else ("nets.%d" % c)
        num, ab = (nZ[:, c].sum(), aZ[:, c].sum()) if c < L else (0, 0)
        z_contribs = [step, en if en is not None else 0]
        put(name + ".bias", num, Dz, (H,), z_contribs, ab)
        put(name + ".weight", num, Dz, (H, H), z_contribs, ab)      # d Z[:, c]^T . Xh, every row of Xh all ones
    if has:
        if variant == "homo":       # d att[q] = H h[q] g / W
            terms = {"h": (H * hs * hs * gq, W * Lk * Lk), "ego": (H * hs * gq * A[:, 0], W * Lk), "b": (H * hs * gq, W * Lk)}
        else:
            terms = {"h": (dsn * hs, W ** 3 * Lk * Lk), "ego": (dsn, W ** 3 * Lk), "b": (dsn, W ** 3 * Lk)}
        wh = _exact_f32(terms["h"][0].sum(), terms["h"][1], (H,))
        we = _exact_f32(terms["ego"][0].sum(), terms["ego"][1], (H,))
        want["attw.weight"] = torch.cat([wh, we]).view(1, 2 * H)
        want["attw.bias"] = _exact_f32(terms["b"][0].sum(), terms["b"][1], (1,))
        for name, key in (("attw.weight[:H]", "h"), ("attw.weight[H:]", "ego"), ("attw.bias", "b")):
            p2 = _pow2_part([terms[key][0]])
            bounds[name] = (p2 / terms[key][1], int(np.abs(terms[key][0]).sum()) // p2)
    return want, bounds, aX != 0


# ---- the comparison -------------------------------------------------------------------------------------------------------
def _rows2d(t):
    t = t.detach().cpu()
    return t.reshape(t.shape[0], -1) if t.dim() > 1 else t.reshape(1, -1)


def differing_rows(got, want):
    g, w = _rows2d(got), _rows2d(want)
    assert g.shape == w.shape, (g.shape, w.shape)
    return torch.nonzero(~(g == w).all(dim=1)).flatten().tolist()


def describe_row(case, n):
    """where row n of X.grad gets its contributions from: the runs of its keys in the sorted DET_ROW sequence with the chunks
    they span, and its positions in sel / egoidx"""
    d = case.data
    keys = scatter_keys(case.variant, d["sel"], d["ids"], d["codes"], case.W, case.L)
    k = np.sort(keys["row"], kind="stable")
    parts = []
    for c in range(case.L):
        at = np.flatnonzero(k == n * case.L + c)
        if len(at):
            parts.append("code %d: DET_ROW run [%d, %d) of K = %d, chunks %d..%d" % (c, at[0], at[-1] + 1, len(k), at[0] // DET_CHUNK,
                                                                                    at[-1] // DET_CHUNK))
    parts.append("%d times in sel" % int((keys["sel"] == n).sum()))
    if case.variant == "hetero":
        parts.append("%d times in egoidx" % int((keys["ego"] == n).sum()))
    parts.append("DET_ROW classes of the batch: %s" % sorted(chunk_classes(k, len(k))))
    return "; ".join(parts)


def compare(case, got, want, touched=None):
    """[] or one message per tensor that differs: the first differing (row, column), got, want and -- for X.grad -- the runs
    and chunks of that row's keys.  With `touched`, the rows of X.grad that nothing touches must be +0 bit for bit."""
    msgs = []
    for name, w in want.items():
        g = got[name].detach().cpu()
        rows = differing_rows(g, w)
        if rows:
            g2, w2 = _rows2d(g), _rows2d(w)
            r = rows[0]
            col = int(torch.nonzero(~(g2[r] == w2[r])).flatten()[0])
            msg = "%s: %d rows differ, first at (row %d, column %d): got %r, want %r" % (name, len(rows), r, col, g2[r, col].item(),
                                                                                        w2[r, col].item())
            if name == "X":
                msg += " [%s]" % describe_row(case, r)
            msgs.append(msg)
    if touched is not None:
        bits = got["X"].detach().cpu().contiguous().view(torch.int32)[torch.from_numpy(~touched)]
        bad = torch.nonzero(bits.any(dim=1)).flatten()
        if len(bad):
            msgs.append("X: untouched row %d is not +0" % int(np.flatnonzero(~touched)[int(bad[0])]))
    return msgs


# ---- a model of the two passes, for the tables' own test ------------------------------------------------------------------
DET_FAULTS = ("a middle chunk taken for a head", "a head at a chunk's first position taken for a middle chunk",
              "the last lead piece of a crossing run left out", "a trail piece added in pass 1 as well")


def model_det_scatter(keys, values, rows, chunk=DET_CHUNK, fault=None):
    """det_scatter_kernel's two passes over the stably sorted (key, value) pairs, restated in integers: -> dst [rows].
    fault: one of DET_FAULTS, a wrong kernel that stays inside any tolerance relative to the tensor's norm."""
    order = np.argsort(np.asarray(keys), kind="stable")
    k, v = np.asarray(keys)[order], np.asarray(values, dtype=np.int64)[order]
    K, nch = len(k), -(-len(k) // chunk)
    dst, cpart = np.zeros(rows, np.int64), np.zeros((nch, 2), np.int64)
    for c in range(nch):                                            # pass 1
        b, e = c * chunk, min(K, (c + 1) * chunk)
        key, acc = k[b], 0
        lead = b > 0 and k[b - 1] == key
        for i in range(b, e):
            if k[i] != key:
                if lead:
                    cpart[c, 0] = acc
                else:
                    dst[key] += acc
                lead, key, acc = False, k[i], 0
            acc += v[i]
        cont = e < K and k[e] == key
        if lead:
            cpart[c, 0] = acc
        elif cont:
            cpart[c, 1] = acc
            if fault == DET_FAULTS[3]:
                dst[key] += acc
        else:
            dst[key] += acc
    for c in range(nch):                                            # pass 2
        b, e = c * chunk, min(K, (c + 1) * chunk)
        key = k[e - 1]
        if not (e < K and k[e] == key):
            continue
        middle = k[b] == key and b > 0 and (k[b - 1] == key or fault == DET_FAULTS[1])
        if middle and fault != DET_FAULTS[0]:
            continue
        acc, c2 = cpart[c, 1], c + 1
        while True:
            e2 = min(K, (c2 + 1) * chunk)
            last = k[e2 - 1] != key or not (e2 < K and k[e2] == key)
            if not (last and fault == DET_FAULTS[2]):
                acc += cpart[c2, 0]
            if last:
                break
            c2 += 1
        dst[key] += acc
    return dst
