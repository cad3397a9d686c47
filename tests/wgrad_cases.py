"""Cases, edge classes and probes for the recurrent weight-gradient GEMMs

    [g_W_ih | g_W_hh] [G H, 2H] = dG^T . [x | h],   g_b = colsum(dG)        over the R = groups W L rows of a micro-batch

(wgradh_kernel of pn_seqh.hip, wgrad4_kernel of pn_seq4.hip, wgrad3_kernel and wgrad_reduce_kernel of pn_seq3.hip, the split
arithmetic of ws_layout / run_wgrad in pn_pagg.hip).  Shared by tests/test_wgrad_cases_host.py, which proves the tables on
the CPU, and tests/test_gpu_wgrad_edges.py, which runs them through the library against the fp64 oracle.

What the kernels do, restated here in plain integers (the constants are read out of the sources; a pattern that stops
matching fails the import):

  rows      row r of the reduction is path step (q, t) of the micro-batch, r = q L + t (xh and dG are [P][L][.]: the BPTT
            writes dG at (tile_row + row L + t) GH, tile_row = q0 L).  For the homo and PAGG plans sequence slot q belongs to
            pooling group q // W, so group s of micro-batch [g0, g1) owns the W L contiguous rows from (s - g0) W L; the
            hetero plan pools q mod S: its groups are not contiguous and it appears with dense gradients only.
  splits    tiles = ceil(G H / 256) ceil(2H / 256);  cus = 224 while 2 rows GH 2H <= 1.2e11, else 256;
            nz = min(ceil(cus / tiles), ceil(Pb L / 128)) >= 1, Pb the paths of a FULL micro-batch;
            launched = min(nz, ceil(R / kt)), kt = 16 (wgradh, wgrad4) or 32 (wgrad3), R of THIS micro-batch.
  K tiles   split z takes tiles z, z + launched, ...: my_tiles(z) of them.  wgradh / wgrad4 take two per trip (an odd count
            runs a tile of zeros), loads past the end are clamped to row R - 1 and masked; a thread owns 4 consecutive rows
            (8 in wgrad3).
  reduce    lane group zg of four adds splits zg, zg + 4, ...: eight at a time while z + 28 < nsplit, then one at a time;
            micro-batch b > 0 adds to what the earlier ones left (accumulate).

The 256-CU branch (2 rows GH 2H > 1.2e11: about 4.6e5 rows at H = 128) is out of reach of a quick test; it stays with the
Pubmed-scale tests of tests/test_gpu_pagg.py.  Every row here has N <= 400, F <= 48 and at most 224 x 128 = 28 672 (+ one
group) reduction rows."""
import collections
import functools
import os
import re

import numpy as np
import torch

from conftest import ROOT
from oracle import pagg_oracle as po

CSRC = os.path.join(ROOT, "pathnet_amd", "csrc")
N, F, C = 400, 48, 5


# ---- constants: restated, and parsed from the sources -----------------------------------------------------------------------
RESTATED = {
    "WG_BM": 256, "WG_BN": 256, "WG_KT": 32,            # wgrad3_kernel (pn_seq.h)
    "WH_BM": 256, "WH_BN": 256, "WH_KT": 16,            # wgradh_kernel (pn_seqh.hip)
    "W4_BM": 256, "W4_BN": 256, "W4_KT": 16,            # wgrad4_kernel (pn_seq4.hip)
    "PN_WGRAD_CUS_SHARED": 224, "CUS_ALL": 256, "FLOPS_SWITCH": 1.2e11,     # ws_layout (pn_pagg.hip)
    "MAX_NZ_ROWS": 4 * 32,                              # max_nz = ceil(rows / (4 WG_KT))
    "REDUCE_GROUPS": 4, "REDUCE_UNROLL": 8,             # wgrad_reduce_kernel (pn_seq3.hip)
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
    m = _find(_src("pn_seq.h"), r"constexpr\s+int\s+WG_BM\s*=\s*(\d+)\s*,\s*WG_BN\s*=\s*(\d+)\s*,\s*WG_KT\s*=\s*(\d+)\s*;", "pn_seq.h WG_*")
    out["WG_BM"], out["WG_BN"], out["WG_KT"] = (int(v) for v in m.groups())
    m = _find(_src("pn_seqh.hip"), r"constexpr\s+int\s+WH_BM\s*=\s*(\d+)\s*,\s*WH_BN\s*=\s*(\d+)\s*,\s*WH_KT\s*=\s*(\d+)\s*,", "pn_seqh.hip WH_*")
    out["WH_BM"], out["WH_BN"], out["WH_KT"] = (int(v) for v in m.groups())
    m = _find(_src("pn_seq4.hip"), r"constexpr\s+int\s+W4_BM\s*=\s*(\d+)\s*,\s*W4_BN\s*=\s*(\d+)\s*,\s*W4_KT\s*=\s*(\d+)\s*,", "pn_seq4.hip W4_*")
    out["W4_BM"], out["W4_BN"], out["W4_KT"] = (int(v) for v in m.groups())
    pagg = _src("pn_pagg.hip")
    out["PN_WGRAD_CUS_SHARED"] = int(_find(pagg, r"#define\s+PN_WGRAD_CUS_SHARED\s+(\d+)", "pn_pagg.hip PN_WGRAD_CUS_SHARED").group(1))
    _find(pagg, r"constexpr\s+int\s+WGRAD_CUS_SHARED\s*=\s*PN_WGRAD_CUS_SHARED\s*;", "pn_pagg.hip WGRAD_CUS_SHARED")
    m = _find(pagg, r"size_t\s+cus\s*=\s*wg_flops\s*<=\s*([0-9.eE+]+)\s*\?\s*WGRAD_CUS_SHARED\s*:\s*(\d+)\s*;", "ws_layout: cus")
    out["FLOPS_SWITCH"], out["CUS_ALL"] = float(m.group(1)), int(m.group(2))
    _find(pagg, r"wg_flops\s*=\s*2\.0\s*\*\s*\(double\)rows\s*\*\s*\(double\)\(G\s*\*\s*H\)\s*\*\s*\(double\)\(2\s*\*\s*H\)\s*;", "ws_layout: wg_flops")
    _find(pagg, r"tiles\s*=\s*std::max<size_t>\(1,\s*\(\(G\s*\*\s*H\s*\+\s*WG_BM\s*-\s*1\)\s*/\s*WG_BM\)\s*\*\s*\(\(2\s*\*\s*H\s*\+\s*WG_BN\s*-\s*1\)\s*/\s*WG_BN\)\)\s*;",
          "ws_layout: tiles")
    _find(pagg, r"size_t\s+nz\s*=\s*\(cus\s*\+\s*tiles\s*-\s*1\)\s*/\s*tiles\s*;", "ws_layout: nz")
    m = _find(pagg, r"max_nz\s*=\s*\(rows\s*\+\s*(\d+)\s*\*\s*WG_KT\s*-\s*1\)\s*/\s*\(\s*(\d+)\s*\*\s*WG_KT\s*\)\s*;", "ws_layout: max_nz")
    assert m.group(1) == m.group(2)
    out["MAX_NZ_ROWS"] = int(m.group(1)) * out["WG_KT"]
    _find(pagg, r"nt16\s*=\s*\(wp\.R\s*\+\s*15\)\s*/\s*16\s*;", "run_wgrad: nt16")
    _find(pagg, r"ntiles\s*=\s*\(wp\.R\s*\+\s*WG_KT\s*-\s*1\)\s*/\s*WG_KT\s*;", "run_wgrad: ntiles")
    red = _src("pn_seq3.hip")
    m = _find(red, r"for\s*\(;\s*z\s*\+\s*(\d+)\s*<\s*nsplit;\s*z\s*\+=\s*(\d+)\)", "wgrad_reduce_kernel: unrolled round")
    ahead, stride = int(m.group(1)), int(m.group(2))
    m = _find(red, r"for\s*\(;\s*z\s*<\s*nsplit;\s*z\s*\+=\s*(\d+)\)", "wgrad_reduce_kernel: tail")
    out["REDUCE_GROUPS"] = int(m.group(1))
    assert stride % out["REDUCE_GROUPS"] == 0 and ahead == stride - out["REDUCE_GROUPS"], (ahead, stride)
    out["REDUCE_UNROLL"] = stride // out["REDUCE_GROUPS"]
    _find(red, r"const\s+int\s+zg\s*=\s*threadIdx\.x\s*>>\s*6\b", "wgrad_reduce_kernel: lane groups")
    return out


PARSED = parse_constants()
KERNELS = ("wgradh", "wgrad4", "wgrad3")
KT = {"wgradh": PARSED["WH_KT"], "wgrad4": PARSED["W4_KT"], "wgrad3": PARSED["WG_KT"]}
TILE_M, TILE_N = PARSED["WG_BM"], PARSED["WG_BN"]
ROWS_PER_THREAD = {"wgradh": 4, "wgrad4": 4, "wgrad3": 8}
TABLES_CUT_FOR = (16, 16, 32, 224)          # the case table below is cut for these K tiles and this CU count


def _cdiv(a, b):
    return -(-a // b)


# ---- the split arithmetic -------------------------------------------------------------------------------------------------
def tiles(H, G):
    return max(1, _cdiv(G * H, TILE_M) * _cdiv(2 * H, TILE_N))


def cus(rows, H, G):
    return PARSED["PN_WGRAD_CUS_SHARED"] if 2.0 * rows * (G * H) * (2 * H) <= PARSED["FLOPS_SWITCH"] else PARSED["CUS_ALL"]


def wgrad_split(Pb, L, H, G):
    """ws_layout's wgrad_split for micro-batches of Pb paths"""
    rows = Pb * L
    return max(1, min(_cdiv(cus(rows, H, G), tiles(H, G)), _cdiv(rows, PARSED["MAX_NZ_ROWS"])))


def launched(R, nz, kt):
    """splits run_wgrad launches (and the reduce adds) for a micro-batch of R rows"""
    return min(nz, _cdiv(R, kt))


def my_tiles(z, R, nsplit, kt):
    """K tiles i = z (mod nsplit) below ceil(R / kt)"""
    nt = _cdiv(R, kt)
    return _cdiv(nt - z, nsplit) if z < nt else 0


def reduce_loops(nsplit):
    """per lane group zg: (trips of the unrolled round, trips of the tail loop) of wgrad_reduce_kernel"""
    g, u = PARSED["REDUCE_GROUPS"], PARSED["REDUCE_UNROLL"]
    out = []
    for zg in range(g):
        z, rounds, tail = zg, 0, 0
        while z + g * (u - 1) < nsplit:
            z, rounds = z + g * u, rounds + 1
        while z < nsplit:
            z, tail = z + g, tail + 1
        out.append((rounds, tail))
    return out


# ---- cases ----------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "variant cell H S W L batch_groups")


def case_id(c):
    return "%s-%s-H%d-S%d-W%d-L%d-bg%d" % (c.variant, cell_of(c), c.H, c.S, c.W, c.L, c.batch_groups)


def cell_of(c):
    return c.cell or ("rnn" if c.variant == "pagg" else "lstm")


def gates(c):
    return 1 if cell_of(c) == "rnn" else 4


def micro_batches(c):
    """[(g0, g1)]: make_dims' Sb and nb"""
    sb = c.batch_groups if 0 < c.batch_groups < c.S else c.S
    return [(g0, min(c.S, g0 + sb)) for g0 in range(0, c.S, sb)]


def rows_of(c, b):
    g0, g1 = micro_batches(c)[b]
    return (g1 - g0) * c.W * c.L


def split_of(c):
    g0, g1 = micro_batches(c)[0]
    return wgrad_split((g1 - g0) * c.W, c.L, c.H, gates(c))


# (seq_math, PN_SEQ4 knob or None: left alone)
ARITHMETICS = (("f16x2", None), ("bf16x3", None), ("bf16x3", 0))


def kernel_of(c, seq_math, seq4):
    """the kernel run_wgrad launches for the case under an arithmetic; None: that parametrization repeats another one"""
    if c.H > 256:                                   # the generic route has no fused arithmetic: wgrad3 whatever seq_math says
        return "wgrad3" if (seq_math, seq4) == ("bf16x3", None) else None
    if seq_math == "f16x2":
        return "wgradh"
    four = c.H == 128 and gates(c) == 4 and 1 <= c.L <= 8          # seq4_select
    if seq4 is None:
        return "wgrad4" if four else "wgrad3"
    return "wgrad3" if four else None               # PN_SEQ4 = 0 changes nothing elsewhere


def runs(c):
    """[(kernel, seq_math, seq4)] of the case"""
    return [(kernel_of(c, sm, k), sm, k) for sm, k in ARITHMETICS if kernel_of(c, sm, k)]


# ---- edge classes ---------------------------------------------------------------------------------------------------------
R_SIZES = ("R < one K tile", "R = one K tile", "R = one K tile + 1", "R mod tile = 1, several tiles", "R mod tile = tile - 1, several tiles",
           "R mod 4 != 0", "R mod 8 != 0")
MY_TILES = ("my_tiles = 1 in every split, several splits", "my_tiles equal and even in every split", "my_tiles equal and odd (> 1) in every split",
            "my_tiles even and odd in one launch (ntiles mod nsplit != 0)")
OWNERS = ("ragged last tile owned by split 0 of >= 3", "ragged last tile owned by the last split of >= 3",
          "ragged last tile owned by a middle split")
REDUCE_NSPLIT = (1, 2, 3, 4, 5, 28, 29, 32, 33, 61)
REDUCE = tuple("reduce over nsplit = %d" % n for n in REDUCE_NSPLIT)
CEILINGS = ("nz = 224, the ceiling of one output tile: H = 32", "nz = 224: H = 64", "nz = 224: the RNN at H = 128",
            "nz = 112, two output tiles: the LSTM at H = 128", "nz = 112: the LSTM at H = 96", "nz = 38, six output tiles: H = 160",
            "nz = 28, eight output tiles: H = 256")
MICRO = ("later micro-batch launches fewer splits than the first (accumulate)", "later micro-batch launches as many splits as the first (accumulate)")
OUT_TILES = ("H = 32: one part-filled output tile", "H = 32, RNN: GH = 32", "H = 96, LSTM: GH = 384, the second M tile half full",
             "H = 128, four gate slots: two full M tiles", "H = 160: H2 = 320, a second N tile of 64 columns (bias sums from blockIdx.x = 0 alone)",
             "H = 256: every output tile full", "GRU: four gate slots, the reduce drops the zero halves and remaps to 3H rows",
             "H = 288: the generic route, GH = 1152, H2 = 576")
ALL_CLASSES = R_SIZES + MY_TILES + OWNERS + REDUCE + CEILINGS + MICRO + OUT_TILES

# what a kernel can meet at all: wgrad4 is built for H = 128 with four gate slots, wgradh for the fused sizes (H <= 256)
_COMMON = R_SIZES + MY_TILES + OWNERS + REDUCE + MICRO
APPLICABLE = {
    "wgradh": _COMMON + CEILINGS + OUT_TILES[:7],
    "wgrad4": _COMMON + (CEILINGS[3], OUT_TILES[3], OUT_TILES[6]),
    "wgrad3": ALL_CLASSES,
}


def _ceiling_class(c):
    H, cell = c.H, cell_of(c)
    if H == 32:
        return CEILINGS[0]
    if H == 64:
        return CEILINGS[1]
    if H == 128 and cell == "rnn":
        return CEILINGS[2]
    if H == 128 and cell == "lstm":
        return CEILINGS[3]
    if H == 96 and cell == "lstm":
        return CEILINGS[4]
    if H == 160 and gates(c) == 4:
        return CEILINGS[5]
    if H == 256 and gates(c) == 4:
        return CEILINGS[6]
    return None


def edge_classes(c, kernel):
    """names (of ALL_CLASSES) of the edges the case contains when `kernel` runs it; empty when it never does"""
    if kernel not in [k for k, _, _ in runs(c)]:
        return set()
    kt, nz, out = KT[kernel], split_of(c), set()
    H, G, cell = c.H, gates(c), cell_of(c)
    counts = []
    for b in range(len(micro_batches(c))):
        R = rows_of(c, b)
        nt, ns = _cdiv(R, kt), launched(R, nz, kt)
        counts.append(ns)
        if R < kt:
            out.add(R_SIZES[0])
        if R == kt:
            out.add(R_SIZES[1])
        if R == kt + 1:
            out.add(R_SIZES[2])
        if R % kt == 1 and nt >= 3:
            out.add(R_SIZES[3])
        if R % kt == kt - 1 and nt >= 3:
            out.add(R_SIZES[4])
        if R % 4:
            out.add(R_SIZES[5])
        if R % 8:
            out.add(R_SIZES[6])
        mine = [my_tiles(z, R, ns, kt) for z in range(ns)]
        assert sum(mine) == nt and min(mine) >= 1
        if ns >= 2 and max(mine) == 1:
            out.add(MY_TILES[0])
        if ns >= 2 and len(set(mine)) == 1 and mine[0] % 2 == 0:
            out.add(MY_TILES[1])
        if ns >= 2 and len(set(mine)) == 1 and mine[0] % 2 == 1 and mine[0] > 1:
            out.add(MY_TILES[2])
        if nt % ns:
            assert len(set(mine)) == 2
            out.add(MY_TILES[3])
        if R % kt and ns >= 3:
            owner = (nt - 1) % ns
            out.add(OWNERS[0] if owner == 0 else OWNERS[1] if owner == ns - 1 else OWNERS[2])
        if ns in REDUCE_NSPLIT:
            out.add("reduce over nsplit = %d" % ns)
        if b == 0 and ns == nz == _cdiv(PARSED["PN_WGRAD_CUS_SHARED"], tiles(H, G)) and _ceiling_class(c):
            out.add(_ceiling_class(c))
    for ns in counts[1:]:
        out.add(MICRO[0] if ns < counts[0] else MICRO[1])
    if H == 32:
        out.add(OUT_TILES[0])
    if H == 32 and cell == "rnn":
        out.add(OUT_TILES[1])
    if H == 96 and cell == "lstm":
        out.add(OUT_TILES[2])
    if H == 128 and G == 4:
        out.add(OUT_TILES[3])
    if H == 160:
        out.add(OUT_TILES[4])
    if H == 256 and G == 4:
        out.add(OUT_TILES[5])
    if cell == "gru":
        out.add(OUT_TILES[6])
    if H == 288:
        out.add(OUT_TILES[7])
    return out


def coverage(cases=None):
    """{kernel: {class: [case ids]}} over the table"""
    cov = {k: {cl: [] for cl in APPLICABLE[k]} for k in KERNELS}
    for c in (CASES if cases is None else cases):
        if c.variant == "hetero":       # dense gradients only: its rows prove no edge on their own
            continue
        for k in KERNELS:
            for cl in edge_classes(c, k):
                if cl in cov[k]:
                    cov[k][cl].append(case_id(c))
    return cov


# ---- the table ------------------------------------------------------------------------------------------------------------
def _c(*a):
    return Case(*a)


# (variant, cell, H, S, W, L, batch_groups); R = rows of the micro-batches, nz = ws_layout's split
CASES = [
    # -- the localized probe rows whose fp32 oracle tests/test_wgrad_cases_host.py holds to the GPU test's own assertion ----
    _c("homo", None, 32, 90, 7, 3, 0),          # R = 1890 = 2 mod 16, mod 32 and mod 4; nz = 15
    _c("homo", "gru", 96, 90, 7, 3, 0),         # the same rows on four gate slots, GH = 384
    _c("pagg", None, 32, 90, 7, 4, 0),          # R = 2520 = 8 mod 16, 24 mod 32; GH = 32
    _c("homo", None, 128, 90, 40, 4, 0),        # R = 14 400: nz = 112, the ceiling of two output tiles
    # -- nz at its ceiling ----------------------------------------------------------------------------------------------
    _c("homo", None, 32, 180, 40, 4, 0),        # R = 28 800: nz = 224, the largest row
    _c("homo", "gru", 64, 180, 40, 4, 0),       # nz = 224 at H = 64 (GH = 256: one full M tile, half an N tile)
    _c("pagg", None, 128, 180, 40, 4, 0),       # nz = 224, the RNN at H = 128 (wgrad3 in bf16 x 3: G = 1)
    _c("homo", None, 96, 90, 40, 4, 0),         # nz = 112, GH = 384
    _c("homo", None, 256, 120, 8, 4, 119),      # R = 3808 / 32: nz = 28 = nsplit, then a micro-batch of two K tiles (one)
    _c("homo", None, 160, 47, 13, 6, 46),       # R = 3588 / 78: nz = 29 below the ceiling of 38; then 5 splits (3 in wgrad3)
    _c("homo", None, 160, 72, 11, 6, 0),        # R = 4752: nz = 38, six output tiles
    # -- reduce counts, my_tiles and owners of the ragged tile at H = 128 (all three kernels) -------------------------------
    _c("homo", "gru", 128, 128, 11, 3, 127),    # R = 4191 / 33: nsplit 33, then 3 (2): every split one tile
    _c("homo", None, 128, 56, 7, 1, 55),        # L = 1: R = 385 / 7: nsplit 4, then one tile of 7 rows
    _c("homo", None, 128, 26, 13, 3, 14),       # R = 546 / 468: nsplit 5 and 5
    _c("homo", None, 128, 33, 1, 1, 17),        # R = 17 / 16: one K tile + 1, then exactly one K tile
    _c("homo", None, 128, 200, 5, 4, 199),      # R = 3980 / 20: nsplit 32, then 2 (1)
    _c("homo", None, 128, 200, 13, 3, 0),       # R = 7800: nsplit 61
    _c("homo", None, 128, 29, 40, 3, 0),        # R = 3480: nsplit 28 below the ceiling
    _c("homo", None, 128, 46, 13, 6, 0),        # R = 3588: nsplit 29
    _c("homo", None, 128, 1, 5, 3, 0),          # R = 15: less than one K tile
    _c("homo", "gru", 128, 97, 7, 4, 40),       # three micro-batches 1120 / 1120 / 476: nsplit 9, 9, 9
    # -- the other output-tile shapes at ragged sizes ---------------------------------------------------------------------
    _c("homo", "rnn", 32, 13, 5, 3, 0),         # GH = 32, R = 195
    _c("homo", "rnn", 64, 31, 3, 1, 16),        # L = 1, R = 48 / 45
    _c("pagg", None, 32, 41, 3, 4, 17),         # PAGG in micro-batches 204 / 204 / 84
    _c("pagg", None, 96, 23, 5, 4, 0),          # RNN at H = 96: GH = 96, R = 460
    _c("homo", None, 96, 37, 5, 3, 19),         # GH = 384, R = 285 / 270
    _c("homo", "gru", 160, 29, 7, 3, 0),        # GRU at H = 160: 3 x 2 output tiles, R = 609
    _c("homo", None, 256, 21, 4, 6, 11),        # H = 256, R = 264 / 240
    _c("homo", None, 288, 1, 1, 1, 0),          # the generic route's smallest launch
    _c("homo", None, 288, 37, 5, 3, 0),         # generic: GH = 1152, H2 = 576 (5 x 3 output tiles), R = 555
    _c("homo", "gru", 288, 37, 5, 3, 19),       # generic GRU in micro-batches
    # -- the hetero plan: dense gradients only -------------------------------------------------------------------------------
    _c("hetero", None, 128, 97, 7, 4, 0),       # R = 2716
    _c("hetero", None, 32, 61, 5, 3, 0),        # R = 915
    _c("hetero", "gru", 96, 45, 11, 6, 20),     # micro-batches 1320 / 1320 / 330
    _c("hetero", None, 160, 33, 8, 4, 0),       # R = 1056
]
CASE_IDS = [case_id(c) for c in CASES]
assert len(set(CASE_IDS)) == len(CASES)
for _k in CASES:
    assert _k.S <= N and max(rows_of(_k, b) for b in range(len(micro_batches(_k)))) <= 224 * 128 + _k.W * _k.L, _k
    assert _k.L in (1, 3, 4, 6) and (_k.variant != "pagg" or _k.L == 4), _k
HOST_ROWS = CASES[:4]


# ---- parameters, inputs, probes -------------------------------------------------------------------------------------------
RECURRENT = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def recurrent_names(c):
    return ["%s.%s" % (cell_of(c).upper(), k) for k in RECURRENT]


def make_params(c, seed=0):
    """a state_dict under the reference's keys from torch's own initialisers (CPU, fp32): what the GPU test loads into the
    module and both oracles read"""
    torch.manual_seed(1000 + seed)
    nn = torch.nn
    H, L = c.H, c.L
    mods = {"fc0": nn.Linear(F, H), "fc2": nn.Linear(2 * H, C)}
    for d in range(4 if c.variant == "pagg" else L):
        mods[("nei%d" % d) if c.variant == "pagg" else ("nets.%d" % d)] = nn.Linear(H, H)
    if c.variant != "pagg":
        mods["attw"] = nn.Linear(2 * H, 1)
    kind = cell_of(c)
    mods[kind.upper()] = {"lstm": nn.LSTM, "gru": nn.GRU, "rnn": nn.RNN}[kind](H, H)
    return {"%s.%s" % (name, k): v.detach().clone() for name, m in mods.items() for k, v in m.state_dict().items()}


def make_inputs(c, seed=0, keep=0.5):
    """X, sel, ids, codes, the explicit dropout masks at keep 0.5 and the dense upstream gradient"""
    g = torch.Generator().manual_seed(seed + 4)
    rng = np.random.default_rng(seed + 1)
    S, W, L, H = c.S, c.W, c.L, c.H
    X = torch.rand(N, F, generator=g)
    sel = np.sort(rng.choice(N, S, replace=False))
    ids = rng.integers(0, N, (S, W, L)).astype(np.int32)
    ids[:, :, 0] = sel[:, None]
    codes = rng.integers(0, L, (S, W, L)).astype(np.uint8)
    mask_seq = (torch.rand(L, S * W, H, generator=g) < keep).float() / keep
    mask_cls = (torch.rand(S, 2 * H, generator=g) < keep).float() / keep
    Gout = torch.randn(S, C, generator=g)
    return dict(X=X, sel=sel, ids=ids, codes=codes, mask_seq=mask_seq, mask_cls=mask_cls, G=Gout)


def straddling_group(c, b, kt):
    """the group of micro-batch b whose rows lie on both sides of the boundary between the last whole K tile and the ragged
    one (None: no ragged tile, no whole tile, or the boundary falls between two groups)"""
    g0, _ = micro_batches(c)[b]
    R, wl = rows_of(c, b), c.W * c.L
    edge = R // kt * kt
    if R % kt == 0 or edge == 0 or edge % wl == 0:
        return None
    return g0 + edge // wl


def probes(c):
    """[(kind, group or None)]: "dense", and for the contiguous plans the one-group gradients -- group 0, the last group, the
    last group of the first micro-batch, the straddling groups of the first and the last micro-batch for either K tile.
    Kinds that name the same group are joined with "+"."""
    out = [("dense", None)]
    if c.variant == "hetero":
        return out
    mb = micro_batches(c)
    want = [("first", 0), ("last", c.S - 1)]
    if len(mb) > 1:
        want.append(("mb0-last", mb[0][1] - 1))
    for b in sorted({0, len(mb) - 1}):
        for kt in sorted(set(KT.values())):
            s = straddling_group(c, b, kt)
            if s is not None:
                want.append(("straddle%d%s" % (kt, "-mb0" if b == 0 and len(mb) > 1 else ""), s))
    by_group = collections.OrderedDict()
    for kind, s in want:
        by_group.setdefault(s, []).append(kind)
    return out + [("+".join(kinds), s) for s, kinds in by_group.items()]


def upstream(c, G, group):
    if group is None:
        return G
    out = torch.zeros_like(G)
    out[group] = G[group]
    return out


def oracle_grads(c, dtype, params=None, inputs=None, which=None):
    """{kind: (logits, {name: grad})} of the CPU oracle in `dtype` for the probes of the case (`which`: a subset of kinds):
    one forward, one backward per probe"""
    params = make_params(c) if params is None else params
    d = make_inputs(c) if inputs is None else inputs
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    out = po.forward(c.variant, leaf, d["X"], d["ids"], d["codes"], d["sel"], c.W, c.L, drop_seq=d["mask_seq"],
                     drop_cls=d["mask_cls"], dtype=dtype, cell=c.cell)
    res = {}
    todo = [(k, s) for k, s in probes(c) if which is None or k in which]
    for kind, s in todo:
        grads = torch.autograd.grad(out, list(leaf.values()), upstream(c, d["G"], s).to(dtype), retain_graph=True, allow_unused=True)
        res[kind] = (out.detach(), {k: (g if g is not None else torch.zeros_like(v)).detach() for (k, v), g in zip(leaf.items(), grads)})
    return res


@functools.lru_cache(maxsize=2)
def reference(cid):
    """the fp64 oracle of a table row, computed once and shared by the arithmetics that run it (read-only)"""
    return oracle_grads(CASES[CASE_IDS.index(cid)], torch.float64)


# ---- the assertion, shared by the GPU test and the host test of the fp32 oracle -------------------------------------------
LOGIT_TOL = 1e-5


def check(c, kind, group, out, grads, want, who):
    """[] or messages: logits within 1e-5 and gradients by tests/gradcheck.py at its default bound against `want` = (logits,
    grads) of the fp64 oracle.  The dense run compares every tensor; a one-group probe compares the logits and the four
    recurrent tensors -- the others are left out by name, none is excused inside the comparison (no zero_ok)."""
    from gradcheck import ZERO_OK_HETERO, assert_grads_close
    want_out, want_g = want
    msgs = []
    out = out.detach().cpu().double()
    err = float((out - want_out.double()).abs().max()) if torch.isfinite(out).all() else float("inf")
    print("%s %s %s: logits off by %.3g" % (who, case_id(c), kind, err))
    if not err < LOGIT_TOL:
        msgs.append("%s: logits off by %g" % (kind, err))
    names = list(want_g) if group is None else recurrent_names(c)
    zero_ok = ZERO_OK_HETERO if (c.variant == "hetero" and group is None) else ()
    try:
        rows = assert_grads_close({k: grads[k] for k in names}, {k: want_g[k] for k in names}, zero_ok=zero_ok,
                                  tag="wgrad_edges|%s|%s|%s" % (who, kind, case_id(c)))
        worst = max((e / m if m > 0 else 0.0) for k, (e, t, m) in rows.items() if k in recurrent_names(c))
        print("%s %s %s: worst error / max |ref| of the recurrent tensors %.3g" % (who, case_id(c), kind, worst))
    except AssertionError as e:
        msgs.append("%s: %s" % (kind, e))
    return msgs
