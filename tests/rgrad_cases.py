"""Cases, edge classes and probes for the row-reduction weight-gradient kernel of the node-level stage

    g_bank_w [L H, H] = dZ'^T . Xh,   g_bank_b = colsum(dZ')          dZ' = dZ gated by Z > 0 for the homo class
    g_fc0_w  [H, F]   = dXh'^T . X,   g_fc0_b  = colsum(dXh')         dXh' = dXh gated by Xh > 0 for the homo class

with the reduction over the R = N rows of the graph (rgrad_kernel, rgrad_pays and launch_rgrad of pn_rgrad.hip; pad_rows_kernel
of pn_plan.hip; run_bank_bwd, run_fc0_bwd and xpad_floats of pn_pagg.hip).  Shared by tests/test_rgrad_cases_host.py, which
proves the tables on the CPU, and tests/test_gpu_rgrad_edges.py, which runs them through the modules against the fp64 oracle.

What the code does, restated here in plain integers (the constants are read out of the sources; a pattern that stops matching
fails the import):

  route     bank: the fixed-order GEMM in deterministic mode, else rgrad_kernel when rgrad_pays(R, M, H), else the atomic GEMM;
            R = N and M = L H for the dense bank, R = the host-side bound of the touched rows and M = H per code for compact
            rows.  fc0: deterministic as above; rgrad_kernel on X itself when F % 4 == 0 and rgrad_pays(N, H, F); on a copy of
            X whose rows are padded to F4 = F rounded up to 4 (pad_rows_kernel, the xpad workspace slot) when xpad_floats > 0
            and rgrad_pays(N, H, F4); else the atomic GEMM.  (Prepared sparse features take fc0 elsewhere: the GPU test
            switches them off.)
  pays      PN_NODE_RGRAD 0: never.  M % 4 or N % 4: never.  Else R >= 2048, or always under PN_NODE_RGRAD = 2.
  xpad      0 floats when F % 4 == 0, N < 2048 (whatever the knob) or in deterministic mode; else N F4 floats while they stay
            within 256 MB.
  splits    tiles = ceil(M / 128) ceil(N / 128) output tiles, ntiles = ceil(R / 32) K tiles,
            nz = min(max(1, ceil(512 / tiles)), max(1, ntiles // 8)); split z walks K tiles z, z + nz, ...: my_tiles(z) of
            them, two per trip (an odd count runs a tile of zeros), loads past the last tile clamped to it and to row R - 1.
  stores    a thread stages quads of columns guarded by c_ok; the first N columns of a pitch-F4 operand are stored at
            ldc = F; the bias sums come from column block 0 alone.

Kernel instantiations: "gate" = rgrad_kernel<GATE, no LIST> (PathNet_homo), "nogate" = rgrad_kernel<no GATE, no LIST> (PAGG
and PathNet).  PAGG has four distance layers, so the no-gate rows with probes have L = 4; the hetero rows (PathNet) carry
L = 1 and L = 3 with the dense gradient only, because their plan is not contiguous."""
import collections
import functools
import os
import re

import numpy as np
import torch

from conftest import ROOT
from oracle import pagg_oracle as po

CSRC = os.path.join(ROOT, "pathnet_amd", "csrc")
C = 5
KNOB_DEFAULT, KNOB_ALWAYS = 1, 2


# ---- constants: restated, and parsed from the sources -----------------------------------------------------------------------
RESTATED = {
    "R_BM": 128, "R_BN": 128, "R_KT": 32,                   # rgrad_kernel
    "SPLIT_WORKGROUPS": 512, "SPLIT_MIN_TILES": 8,          # launch_rgrad: nz
    "PAYS_ROWS": 2048,                                      # rgrad_pays
    "XPAD_MIN_NODES": 2048, "XPAD_CAP_BYTES": 256 << 20,    # xpad_floats
}


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _find(txt, pattern, what):
    m = re.search(pattern, txt)
    assert m, "%s: the source no longer matches %r" % (what, pattern)
    return m


def parse_constants():
    """the same names as RESTATED, read out of the sources"""
    out = {}
    rg = _src("pn_rgrad.hip")
    m = _find(rg, r"constexpr\s+int\s+R_BM\s*=\s*(\d+)\s*,\s*R_BN\s*=\s*(\d+)\s*,\s*R_KT\s*=\s*(\d+)\s*,", "pn_rgrad.hip R_*")
    out["R_BM"], out["R_BN"], out["R_KT"] = (int(v) for v in m.groups())
    _find(rg, r"tiles\s*=\s*\(\(p\.M\s*\+\s*R_BM\s*-\s*1\)\s*/\s*R_BM\)\s*\*\s*\(\(p\.N\s*\+\s*R_BN\s*-\s*1\)\s*/\s*R_BN\)\s*;", "launch_rgrad: tiles")
    _find(rg, r"ntiles\s*=\s*\(p\.R\s*\+\s*R_KT\s*-\s*1\)\s*/\s*R_KT\s*;", "launch_rgrad: ntiles")
    m = _find(rg, r"nz\s*=\s*std::max<int64_t>\(1,\s*\((\d+)\s*\+\s*tiles\s*-\s*1\)\s*/\s*tiles\)\s*;", "launch_rgrad: nz, the tile term")
    out["SPLIT_WORKGROUPS"] = int(m.group(1))
    m = _find(rg, r"nz\s*=\s*std::min\(nz,\s*std::max<int64_t>\(1,\s*ntiles\s*/\s*(\d+)\)\)\s*;", "launch_rgrad: nz, the K term")
    out["SPLIT_MIN_TILES"] = int(m.group(1))
    _find(rg, r"my_tiles\s*=\s*\(int64_t\)blockIdx\.z\s*<\s*ntiles\s*\?\s*\(ntiles\s*-\s*blockIdx\.z\s*\+\s*nz\s*-\s*1\)\s*/\s*nz\s*:\s*0\s*;", "rgrad_kernel: my_tiles")
    _find(rg, r"\(blockIdx\.z\s*\+\s*std::min\(i,\s*my_tiles\s*-\s*1\)\s*\*\s*nz\)\s*\*\s*R_KT", "rgrad_kernel: row0_of")
    _find(rg, r"if\s*\(knobs_of\(ctx\)\.node_rgrad\s*==\s*0\)\s*return\s+false\s*;", "rgrad_pays: knob 0")
    _find(rg, r"if\s*\(M\s*%\s*4\s*!=\s*0\s*\|\|\s*N\s*%\s*4\s*!=\s*0\)\s*return\s+false\s*;", "rgrad_pays: quads")
    m = _find(rg, r"return\s+R\s*>=\s*(\d+)\s*\|\|\s*knobs_of\(ctx\)\.node_rgrad\s*==\s*2\s*;", "rgrad_pays: rows")
    out["PAYS_ROWS"] = int(m.group(1))
    pagg = _src("pn_pagg.hip")
    m = _find(pagg, r"if\s*\(d\.F\s*%\s*4\s*==\s*0\s*\|\|\s*d\.N\s*<\s*(\d+)\s*\|\|\s*d\.det\)\s*return\s+0\s*;", "xpad_floats: floor")
    out["XPAD_MIN_NODES"] = int(m.group(1))
    m = _find(pagg, r"return\s+n\s*\*\s*4\s*<=\s*\(\(size_t\)(\d+)\s*<<\s*(\d+)\)\s*\?\s*n\s*:\s*0\s*;", "xpad_floats: cap")
    out["XPAD_CAP_BYTES"] = int(m.group(1)) << int(m.group(2))
    _find(pagg, r"rgrad_pays\(ctx,\s*d\.N,\s*L\s*\*\s*H,\s*H\)", "run_bank_bwd: the dense bank's route")
    _find(pagg, r"d\.F\s*%\s*4\s*==\s*0\s*&&\s*rgrad_pays\(ctx,\s*d\.N,\s*H,\s*d\.F\)", "run_fc0_bwd: the direct route")
    _find(pagg, r"xpad_floats\(d\)\s*>\s*0\s*&&\s*rgrad_pays\(ctx,\s*d\.N,\s*H,\s*\(d\.F\s*\+\s*3\)\s*/\s*4\s*\*\s*4\)", "run_fc0_bwd: the padded route")
    return out


PARSED = parse_constants()
KT, TILE_M, TILE_N = PARSED["R_KT"], PARSED["R_BM"], PARSED["R_BN"]
TABLES_CUT_FOR = (128, 128, 32, 512, 8, 2048, 2048, 256 << 20)      # the case table below is cut for these


def _cdiv(a, b):
    return -(-a // b)


# ---- the rules ------------------------------------------------------------------------------------------------------------
def rgrad_pays(R, M, Ncols, knob):
    if knob == 0 or M % 4 or Ncols % 4:
        return False
    return R >= PARSED["PAYS_ROWS"] or knob == KNOB_ALWAYS


def xpad_floats(N, F, deterministic):
    if F % 4 == 0 or N < PARSED["XPAD_MIN_NODES"] or deterministic:
        return 0
    n = N * _cdiv(F, 4) * 4
    return n if n * 4 <= PARSED["XPAD_CAP_BYTES"] else 0


def padded_hidden(H):
    """the hidden size the kernels run at (the modules pad to a multiple of 32)"""
    return _cdiv(H, 32) * 32


def route(variant, N, F, H, L, knob=KNOB_DEFAULT, deterministic=False, compact=0):
    """{"g_bank_w": r, "g_fc0_w": r}, r one of "rgrad", "rgrad+xpad", "gemm", "det".  compact: 0 for the dense bank, else the
    host-side bound of the touched rows (min(N, rows of Z)), which is what the per-code launches reduce over.  The variant
    selects the GATE instantiation, not the route."""
    assert variant in po.VARIANTS
    H = padded_hidden(H)
    if deterministic:
        return {"g_bank_w": "det", "g_fc0_w": "det"}
    bank = rgrad_pays(compact, H, H, knob) if compact else rgrad_pays(N, L * H, H, knob)
    if F % 4 == 0 and rgrad_pays(N, H, F, knob):
        fc0 = "rgrad"
    elif xpad_floats(N, F, deterministic) > 0 and rgrad_pays(N, H, _cdiv(F, 4) * 4, knob):
        fc0 = "rgrad+xpad"
    else:
        fc0 = "gemm"
    return {"g_bank_w": "rgrad" if bank else "gemm", "g_fc0_w": fc0}


def out_tiles(M, Ncols):
    return _cdiv(M, TILE_M) * _cdiv(Ncols, TILE_N)


def nz(R, M, Ncols):
    """launch_rgrad's K split"""
    n = max(1, _cdiv(PARSED["SPLIT_WORKGROUPS"], out_tiles(M, Ncols)))
    return min(n, max(1, _cdiv(R, KT) // PARSED["SPLIT_MIN_TILES"]))


def my_tiles(z, R, nsplit):
    """K tiles i = z (mod nsplit) below ceil(R / 32)"""
    nt = _cdiv(R, KT)
    return _cdiv(nt - z, nsplit) if z < nt else 0


def ragged_owner(R, nsplit):
    """the split that walks the ragged last K tile (None: R is a multiple of the tile)"""
    return (_cdiv(R, KT) - 1) % nsplit if R % KT else None


# ---- cases ----------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "variant cell N F H L S W knob batch_groups")
GEMMS = ("g_bank_w", "g_fc0_w")
INSTANTIATIONS = ("gate", "nogate")


def case_id(c):
    return "%s-%s-N%d-F%d-H%d-L%d-S%d-W%d-knob%d-bg%d" % (c.variant, cell_of(c), c.N, c.F, c.H, c.L, c.S, c.W, c.knob, c.batch_groups)


def cell_of(c):
    return c.cell or ("rnn" if c.variant == "pagg" else "lstm")


def instantiation(c):
    return "gate" if c.variant == "homo" else "nogate"


def micro_batches(c):
    """[(g0, g1)]: make_dims' Sb and nb"""
    sb = c.batch_groups if 0 < c.batch_groups < c.S else c.S
    return [(g0, min(c.S, g0 + sb)) for g0 in range(0, c.S, sb)]


def route_of(c):
    return route(c.variant, c.N, c.F, c.H, c.L, c.knob, False, 0)


def gemm_shape(c, which):
    """(R, M, Ncols) of the launch: Ncols is the stored width, the padded route reads F4 columns"""
    return (c.N, c.L * c.H, c.H) if which == "g_bank_w" else (c.N, c.H, c.F)


def nz_of(c, which):
    R, M, Nc = gemm_shape(c, which)
    return nz(R, M, Nc)


# ---- edge classes ---------------------------------------------------------------------------------------------------------
R_SIZES = ("R < one K tile", "R = 32", "R = 33", "R mod 32 = 1, several tiles, odd tile count", "R mod 32 = 31, even tile count")
SPLITS = ("nz = 2, equal even shares", "nz = 2, an odd share, ragged tile owned by split 0", "ragged tile owned by the last split",
          "nz = 3", "the tile term ceil(512 / tiles) binds, ntiles / 8 does not")
OUT_M = ("M = H = 32: a quarter tile", "M = H = 96", "M = H = 128: one full tile", "M = H = 160: the second M tile a quarter full")
BANK_M_GATE = ("bank M = L H = 32 (L = 1)", "bank M = 3 x 96 = 288", "bank M = 4 x 128 = 512")
BANK_M_NOGATE = ("bank M = 4 x 32 = 128", "bank M = 4 x 96 = 384", "bank M = 4 x 128 = 512", "bank M = 4 x 160 = 640")
COLS = ("F = 4, direct", "F = 8, direct", "F = 128, direct", "F = 132, direct: the second column tile has one quad")
PADDED = ("F = 5, padded", "F = 127, padded", "F = 129, padded: one stored column of the second tile's one quad, odd ldc")
# asked of the table once, whichever instantiation carries them
ONCE = ("Cora's F = 1433 at N = 2708, padded", "N = 2047 under the default knob: the GEMM", "N = 2048 under the default knob: the kernel",
        "three micro-batches accumulate before the one reduction")
ALL_CLASSES = tuple(dict.fromkeys(R_SIZES + SPLITS + OUT_M + BANK_M_GATE + BANK_M_NOGATE + COLS + PADDED + ONCE))
_COMMON = R_SIZES + SPLITS + OUT_M + COLS + PADDED
APPLICABLE = {"gate": _COMMON + BANK_M_GATE, "nogate": _COMMON + BANK_M_NOGATE}


def edge_classes(c):
    """names (of ALL_CLASSES) of the edges the case contains"""
    out, rt = set(), route_of(c)
    R, H, L, F = c.N, c.H, c.L, c.F
    on_kernel = [g for g in GEMMS if rt[g] != "gemm"]
    if c.N == 2047 and c.knob == KNOB_DEFAULT and not on_kernel:
        out.add(ONCE[1])
    if not on_kernel:
        return out
    nt = _cdiv(R, KT)
    if R < KT:
        out.add(R_SIZES[0])
    if R == KT:
        out.add(R_SIZES[1])
    if R == KT + 1:
        out.add(R_SIZES[2])
    if R % KT == 1 and nt >= 3 and nt % 2 == 1:
        out.add(R_SIZES[3])
    if R % KT == KT - 1 and nt >= 2 and nt % 2 == 0:
        out.add(R_SIZES[4])
    for g in on_kernel:
        n = nz_of(c, g)
        mine = [my_tiles(z, R, n) for z in range(n)]
        assert sum(mine) == nt and min(mine) >= 1
        own = ragged_owner(R, n)
        if n == 2 and mine[0] == mine[1] and mine[0] % 2 == 0:
            out.add(SPLITS[0])
        if n == 2 and mine[0] % 2 == 1 and own == 0:
            out.add(SPLITS[1])
        if n >= 2 and own == n - 1:
            out.add(SPLITS[2])
        if n == 3:
            out.add(SPLITS[3])
        _, M, Nc = gemm_shape(c, g)
        if n == _cdiv(PARSED["SPLIT_WORKGROUPS"], out_tiles(M, Nc)) < nt // PARSED["SPLIT_MIN_TILES"]:
            out.add(SPLITS[4])
    if H in (32, 96, 128, 160):
        out.add(OUT_M[(32, 96, 128, 160).index(H)])
    if rt["g_bank_w"] == "rgrad":
        name = "bank M = L H = 32 (L = 1)" if (L, H) == (1, 32) else "bank M = %d x %d = %d" % (L, H, L * H)
        if name in ALL_CLASSES:
            out.add(name)
    if rt["g_fc0_w"] == "rgrad" and F in (4, 8, 128, 132):
        out.add(COLS[(4, 8, 128, 132).index(F)])
    if rt["g_fc0_w"] == "rgrad+xpad":
        if F in (5, 127, 129):
            out.add(PADDED[(5, 127, 129).index(F)])
        if (F, c.N) == (1433, 2708):
            out.add(ONCE[0])
    if c.N == 2048 and c.knob == KNOB_DEFAULT:
        out.add(ONCE[2])
    if len(micro_batches(c)) == 3:
        out.add(ONCE[3])
    return out


def coverage(cases=None):
    """({instantiation: {class: [case ids]}}, {class of ONCE: [case ids]}) over the rows that carry probes"""
    cov = {k: {cl: [] for cl in APPLICABLE[k]} for k in INSTANTIATIONS}
    once = {cl: [] for cl in ONCE}
    for c in (CASES if cases is None else cases):
        if c.variant == "hetero":       # dense gradients only: its rows prove no edge on their own
            continue
        for cl in edge_classes(c):
            if cl in cov[instantiation(c)]:
                cov[instantiation(c)][cl].append(case_id(c))
            if cl in once:
                once[cl].append(case_id(c))
    return cov, once


# ---- the table ------------------------------------------------------------------------------------------------------------
def _c(*a):
    return Case(*a)


# (variant, cell, N, F, H, L, S, W, knob, batch_groups); R = N.  nz: bank / fc0
CASES = [
    # -- GATE: PathNet_homo, the kernel forced below 2 048 rows ---------------------------------------------------------------
    _c("homo", None, 20, 4, 32, 1, 10, 8, 2, 0),            # R < one K tile; M = 32 for both; nz 1 / 1
    _c("homo", None, 32, 8, 96, 3, 12, 3, 2, 0),            # R = 32; bank M = 288
    _c("homo", None, 33, 128, 128, 4, 12, 2, 2, 0),         # R = 33; bank M = 512, one full tile of fc0
    _c("homo", None, 257, 132, 160, 3, 12, 3, 2, 0),        # nine K tiles, the last of one row; M = 160; F = 132
    _c("homo", None, 255, 8, 32, 4, 12, 2, 2, 0),           # eight K tiles, the last of 31 rows
    _c("homo", None, 512, 4, 96, 3, 12, 3, 2, 0),           # nz = 2, eight tiles each
    _c("homo", None, 513, 132, 128, 4, 12, 2, 2, 0),        # nz = 2, nine and eight tiles, split 0 owns the ragged one
    _c("homo", "gru", 545, 8, 160, 1, 12, 8, 2, 0),         # nz = 2, nine tiles each, split 1 owns the ragged one; L = 1
    _c("homo", None, 773, 128, 32, 3, 12, 3, 2, 0),         # nz = 3: nine, eight, eight
    _c("homo", None, 6001, 8, 256, 6, 12, 9, 1, 0),         # bank: 24 output tiles, nz = 22 of 188 K tiles; fc0 nz = 23
    _c("homo", None, 2048, 5, 32, 3, 12, 5, 1, 0),          # padded: F4 = 8; nz = 8 / 8
    _c("homo", None, 2048, 127, 128, 4, 12, 4, 1, 0),       # padded: F4 = 128
    _c("homo", None, 2048, 129, 96, 3, 12, 5, 1, 0),        # padded: F4 = 132, ldc = 129
    _c("homo", None, 2708, 1433, 128, 4, 12, 5, 1, 0),      # Cora's feature width: F4 = 1436, 12 column tiles; nz 10 / 10
    _c("homo", None, 2047, 8, 32, 3, 12, 5, 1, 0),         # the default knob one row short of the kernel: the atomic GEMM
    _c("homo", None, 2048, 8, 32, 3, 12, 5, 1, 0),          # ... and at it: nz = 8
    # -- no GATE: PAGG (four distance layers) -------------------------------------------------------------------------------
    _c("pagg", None, 20, 4, 32, 4, 10, 2, 2, 0),
    _c("pagg", None, 32, 8, 96, 4, 12, 2, 2, 0),
    _c("pagg", None, 33, 132, 128, 4, 12, 2, 2, 0),
    _c("pagg", None, 257, 128, 160, 4, 12, 2, 2, 0),
    _c("pagg", None, 255, 4, 96, 4, 12, 2, 2, 0),
    _c("pagg", None, 512, 8, 32, 4, 12, 2, 2, 0),
    _c("pagg", None, 513, 128, 128, 4, 30, 2, 2, 12),       # three micro-batches of 12 / 12 / 6 groups
    _c("pagg", None, 545, 132, 160, 4, 12, 2, 2, 0),
    _c("pagg", None, 773, 4, 32, 4, 12, 3, 2, 0),
    _c("pagg", None, 8500, 8, 256, 4, 12, 18, 1, 0),        # bank: 16 output tiles, nz = 32 of 266 K tiles; fc0 nz = 33
    _c("pagg", None, 2048, 5, 96, 4, 12, 4, 1, 0),
    _c("pagg", None, 2048, 127, 32, 4, 12, 4, 1, 0),
    _c("pagg", None, 2048, 129, 128, 4, 12, 4, 1, 0),
    # -- no GATE: PathNet, dense gradients only -------------------------------------------------------------------------------
    _c("hetero", None, 513, 8, 96, 3, 12, 3, 2, 0),
    _c("hetero", None, 773, 132, 32, 1, 12, 8, 2, 0),
    _c("hetero", None, 2048, 129, 128, 4, 30, 4, 1, 12),    # padded, three micro-batches
]
CASE_IDS = [case_id(c) for c in CASES]
assert len(set(CASE_IDS)) == len(CASES)
# at least one row per route: rgrad for both tensors, rgrad + rgrad+xpad, gemm for both
HOST_ROWS = [CASES[6], CASES[12], CASES[14], CASES[22], CASES[27]]


# ---- parameters, inputs, probes -------------------------------------------------------------------------------------------
def bank_names(c):
    return [("nei%d" % d) if c.variant == "pagg" else ("nets.%d" % d) for d in range(c.L)]


def node_level_names(c):
    """what rgrad_kernel (or the GEMM in its place) writes: fc0 and the distance bank"""
    return ["fc0.weight", "fc0.bias"] + ["%s.%s" % (b, k) for b in bank_names(c) for k in ("weight", "bias")]


def make_params(c, seed=0):
    """a state_dict under the reference's keys from torch's own initialisers (CPU, fp32): what the GPU test loads into the
    module and both oracles read"""
    torch.manual_seed(1000 + seed)
    nn = torch.nn
    H, L = c.H, c.L
    assert c.variant != "pagg" or L == 4
    mods = {"fc0": nn.Linear(c.F, H), "fc2": nn.Linear(2 * H, C)}
    for b in bank_names(c):
        mods[b] = nn.Linear(H, H)
    if c.variant != "pagg":
        mods["attw"] = nn.Linear(2 * H, 1)
    kind = cell_of(c)
    mods[kind.upper()] = {"lstm": nn.LSTM, "gru": nn.GRU, "rnn": nn.RNN}[kind](H, H)
    return {"%s.%s" % (name, k): v.detach().clone() for name, m in mods.items() for k, v in m.state_dict().items()}


def edge_nodes(c):
    """the reduction rows on an edge, ascending: node 0, 31 / 32, N - 1, the first and last row of the ragged tile, and for
    each GEMM of the row one node in a tile owned by each split z -- the middle tile of an even split's walk, the last tile
    of an odd split's (after which an odd count runs the tile of zeros and the clamped re-load)"""
    R = c.N
    out = {0, R - 1, min(31, R - 1), min(32, R - 1)}
    if R % KT:
        out.add(R // KT * KT)
    for g in GEMMS:
        n = nz_of(c, g)
        for z in range(n):
            mine = my_tiles(z, R, n)
            tile = z + n * (mine - 1 if z % 2 else mine // 2)
            out.add(min(tile * KT + (5 * z + 3) % KT, R - 1))
    return sorted(out)


def split_nodes(c, which):
    """{z: edge nodes in a K tile that split z of the GEMM walks}"""
    n = nz_of(c, which)
    got = {z: [] for z in range(n)}
    for e in edge_nodes(c):
        got[(e // KT) % n].append(e)
    return got


def make_inputs(c, seed=0, keep=0.5):
    """X, sel, ids, codes, the explicit dropout masks at keep 0.5 and the dense upstream gradient.  For the contiguous plans
    masked node 0 is node 0 and the last one node N - 1, and the paths of those two groups are pinned: every slot of theirs
    visits a node of edge_nodes(c), all of them at least once -- the first group under codes that cycle through every
    distance layer, the last under codes 0 and L - 1 alone (the layers between have an exactly zero reference there)."""
    g = torch.Generator().manual_seed(seed + 4)
    rng = np.random.default_rng(seed + 1)
    N, S, W, L, H = c.N, c.S, c.W, c.L, c.H
    X = torch.rand(N, c.F, generator=g)
    if c.variant == "hetero":
        sel = np.sort(rng.choice(N, S, replace=False))
    else:
        sel = np.concatenate([[0], np.sort(rng.choice(np.arange(1, N - 1), S - 2, replace=False)), [N - 1]])
    ids = rng.integers(0, N, (S, W, L)).astype(np.int32)
    ids[:, :, 0] = sel[:, None]
    codes = rng.integers(0, L, (S, W, L)).astype(np.uint8)
    if c.variant != "hetero":
        edges = np.asarray(edge_nodes(c))
        E, j = len(edges), np.arange(W * L)
        assert W * L >= E, (case_id(c), W * L, E)
        ids[0] = edges[j % E].reshape(W, L)
        codes[0] = ((j + j // max(E, L)) % L).reshape(W, L)
        ids[S - 1] = edges[(E - 1 - j) % E].reshape(W, L)
        codes[S - 1] = np.where((j + j // max(E, L)) % 2 == 0, 0, L - 1).reshape(W, L)
    mask_seq = (torch.rand(L, S * W, H, generator=g) < keep).float() / keep
    mask_cls = (torch.rand(S, 2 * H, generator=g) < keep).float() / keep
    Gout = torch.randn(S, C, generator=g)
    return dict(X=X, sel=sel, ids=ids, codes=codes, mask_seq=mask_seq, mask_cls=mask_cls, G=Gout)


def probes(c):
    """[(kind, group or None)]: "dense", and for the contiguous plans the two pinned one-group gradients"""
    out = [("dense", None)]
    if c.variant != "hetero":
        out += [("first", 0), ("last", c.S - 1)]
    return out


def upstream(c, G, group):
    if group is None:
        return G
    out = torch.zeros_like(G)
    out[group] = G[group]
    return out


def oracle_grads(c, dtype, params=None, inputs=None, which=None, return_intermediates=False):
    """{kind: (logits, {name: grad})} of the CPU oracle in `dtype` for the probes of the case (`which`: a subset of kinds):
    one forward, one backward per probe.  return_intermediates: also {kind: (dXh, dy)} -- the gradients at the oracle's Xh
    [N, H] and bank output y [P, L, H] -- and the forward's own intermediates."""
    params = make_params(c) if params is None else params
    d = make_inputs(c) if inputs is None else inputs
    leaf = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in params.items()}
    out, mid = po.forward(c.variant, leaf, d["X"], d["ids"], d["codes"], d["sel"], c.W, c.L, drop_seq=d["mask_seq"],
                          drop_cls=d["mask_cls"], dtype=dtype, cell=c.cell, return_intermediates=True)
    res, inner = {}, {}
    todo = [(k, s) for k, s in probes(c) if which is None or k in which]
    for kind, s in todo:
        targets = list(leaf.values()) + ([mid["Xh"], mid["y"]] if return_intermediates else [])
        grads = torch.autograd.grad(out, targets, upstream(c, d["G"], s).to(dtype), retain_graph=True, allow_unused=True)
        res[kind] = (out.detach(), {k: (g if g is not None else torch.zeros_like(v)).detach() for (k, v), g in zip(leaf.items(), grads)})
        if return_intermediates:
            inner[kind] = (grads[-2].detach(), grads[-1].detach())
    if return_intermediates:
        return res, inner, {k: v.detach() for k, v in mid.items() if v is not None}
    return res


@functools.lru_cache(maxsize=2)
def reference(cid):
    """the fp64 oracle of a table row, computed once (read-only)"""
    return oracle_grads(CASES[CASE_IDS.index(cid)], torch.float64)


# ---- the assertion, shared by the GPU test and the host tests --------------------------------------------------------------
LOGIT_TOL = 1e-5


def check(c, kind, group, out, grads, want, who, shares=None):
    """[] or messages: logits within 1e-5 and gradients by tests/gradcheck.py at its default bound against `want` = (logits,
    grads) of the fp64 oracle.  The dense run compares every tensor; a one-group probe compares the logits and the
    node-level tensors -- the others are left out by name, none is excused inside the comparison (no zero_ok).  Prints, per
    GEMM and its route, the worst error / max |ref|; shares (a list) collects error / tolerance of the node-level tensors."""
    from gradcheck import ZERO_OK_HETERO, assert_grads_close
    want_out, want_g = want
    msgs = []
    out = out.detach().cpu().double()
    err = float((out - want_out.double()).abs().max()) if torch.isfinite(out).all() else float("inf")
    print("%s %s %s: logits off by %.3g" % (who, case_id(c), kind, err))
    if not err < LOGIT_TOL:
        msgs.append("%s: logits off by %g" % (kind, err))
    names = list(want_g) if group is None else node_level_names(c)
    zero_ok = ZERO_OK_HETERO if (c.variant == "hetero" and group is None) else ()
    try:
        rows = assert_grads_close({k: grads[k] for k in names}, {k: want_g[k] for k in names}, zero_ok=zero_ok,
                                  tag="rgrad_edges|%s|%s|%s" % (who, kind, case_id(c)))
        rt = route_of(c)
        for gemm, mine in (("g_fc0_w", ["fc0.weight", "fc0.bias"]), ("g_bank_w", node_level_names(c)[2:])):
            worst = max((rows[k][0] / rows[k][2] if rows[k][2] > 0 else 0.0) for k in mine)
            print("%s %s %s: %s on %s worst error / max |ref| %.3g" % (who, case_id(c), kind, gemm, rt[gemm], worst))
        if shares is not None:
            shares += [rows[k][0] / rows[k][1] for k in node_level_names(c) if rows[k][1] > 0]
    except AssertionError as e:
        msgs.append("%s: %s" % (kind, e))
    return msgs
