"""CPU-side checks of the walk statistics (pn_stats.hip): the interface is declared, exported and bound without an ABI bump,
sized without a device, and refuses bad arguments before a device is needed; and the NumPy restatement the GPU tests
compare against (walk_stats_ref.py) is itself checked against numbers worked out by hand and against the goldens."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import walk_stats_ref
from conftest import ROOT, golden, golden_files
from pathnet_amd import _lib

NEW = ("pn_walk_stats_workspace_bytes", "pn_walk_stats")
FAKE = ctypes.c_void_p(4096)      # a non-null pointer that is never followed: every call below fails before any launch


def test_walk_stats_symbols_are_declared_exported_and_bound_at_abi_12():
    txt = open(os.path.join(ROOT, "include", "pathnet_hip.h")).read()
    lib = _lib.load()
    bare = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
        proto = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, bare, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name][1]), name
    m = re.search(r"typedef struct pn_walk_stats_out \{(.*?)\} pn_walk_stats_out;", bare, re.S)
    assert m, "pn_walk_stats_out"
    fields = re.findall(r"int(?:64|32)_t\s*\*\s*(\w+);", m.group(1))
    assert tuple(fields) == _lib.WalkStatsOut.FIELDS == walk_stats_ref.FIELDS
    assert ctypes.sizeof(_lib.WalkStatsOut) == 8 * len(fields)
    from pathnet_amd import WalkStats, walkstats
    assert WalkStats._fields == tuple(fields) and callable(walkstats.walk_stats)
    declared = int(re.search(r"#define PN_ABI_VERSION (\d+)", txt).group(1))
    assert lib.pn_abi_version() == declared == _lib.ABI_VERSION == 12


def test_workspace_query_needs_no_device_and_accepts_the_limits_themselves():
    lib = _lib.load()
    for n, W, L, rows, C in ((183, 40, 4, 366, 5), (1, 1, 1, 0, 0), (10, 512, 16, 3, 64), (10, 8192, 1, 1, 1),
                             (2 ** 31 - 1, 1024, 8, 1 << 40, 0)):
        b = ctypes.c_int64(-1)
        _lib.check(lib.pn_walk_stats_workspace_bytes(n, W, L, rows, C, ctypes.byref(b)))
        assert 0 <= b.value <= 1 << 20
    assert lib.pn_walk_stats_workspace_bytes(10, 4, 4, 1, 0, None) == _lib.PN_ERR_ARG


CASES = ["L<1", "L>16", "W<1", "W*L>8192", "W*L overflows int32", "C<1 with labels", "C>64 with labels", "rows<0", "n<1",
         "null out", "label_pairs without labels", "unlabeled without labels", "null ids", "null codes"]


@pytest.mark.parametrize("case", CASES)
def test_bad_arguments_are_refused_without_a_device(case):
    lib = _lib.load()
    n, W, L, rows, C = 10, 5, 4, 3, 3
    ids, codes, labels = FAKE, FAKE, FAKE
    out = _lib.WalkStatsOut(*([FAKE.value] * len(_lib.WalkStatsOut.FIELDS)))
    outp = ctypes.byref(out)
    shape_error = True
    if case == "L<1":
        L = 0
    elif case == "L>16":
        L = 17
    elif case == "W<1":
        W = 0
    elif case == "W*L>8192":
        W, L = 8193 // 16 + 1, 16       # 513 * 16 = 8208
    elif case == "W*L overflows int32":
        W, L = 2 ** 31 - 1, 16
    elif case == "C<1 with labels":
        C, shape_error = 0, False       # the query takes C = 0 as "no labels"
    elif case == "C>64 with labels":
        C = 65
    elif case == "rows<0":
        rows = -1
    elif case == "n<1":
        n = 0
    else:
        shape_error = False
        if case == "null out":
            outp = None
        elif case == "null ids":
            ids = None
        elif case == "null codes":
            codes = None
        else:
            labels = None
            for f in ("label_pairs", "unlabeled"):
                if not case.startswith(f):
                    setattr(out, f, None)
    rc = lib.pn_walk_stats(None, n, W, L, rows, ids, codes, None, labels, C, 0, outp, None, 0, None)
    assert rc == _lib.PN_ERR_ARG, (case, rc)
    assert lib.pn_last_error()
    b = ctypes.c_int64(0)
    want = _lib.PN_ERR_ARG if shape_error else _lib.PN_OK
    assert lib.pn_walk_stats_workspace_bytes(n, W, L, rows, C, ctypes.byref(b)) == want, case


def test_python_surface_refuses_bad_calls_before_it_touches_the_device():
    from pathnet_amd import walkstats
    ids = np.zeros((2, 3, 4), np.int32)
    with pytest.raises(ValueError, match="exclude"):
        walkstats.walk_stats(ids, ids, 5, accumulate_into=walkstats.WalkStats(*[None] * 10),
                             out=walkstats.WalkStats(*[None] * 10))
    with pytest.raises(ValueError, match=r"\[\.\.\., W, L\]"):
        walkstats.walk_stats(np.zeros(4, np.int32), np.zeros(4, np.uint8), 5)
    assert walkstats.main(["only", "two"]) == 2


# ---- the restatement itself ------------------------------------------------------------------------------------------

def test_restatement_on_a_case_worked_out_by_hand():
    """2 rows x 3 paths x 3 steps over 6 nodes; the second row holds an id outside the graph with a code >= L, a repeated
    path and an unlabelled node."""
    ids = np.array([[[0, 1, 2], [0, 1, 0], [0, 0, 1]],
                    [[3, 4, 4], [3, 4, 4], [3, 7, 3]]], np.int32)
    codes = np.array([[[0, 1, 2], [0, 1, 0], [0, 0, 1]],
                      [[0, 1, 1], [0, 1, 1], [0, 5, 0]]], np.uint8)
    labels = np.array([0, 1, 0, 1, -1, 0])
    r = walk_stats_ref.walk_stats(ids, codes, 6, labels=labels, num_classes=2)
    assert r.step_code.tolist() == [[6, 0, 0], [1, 4, 0], [2, 3, 1]]
    assert r.counters.tolist() == [1, 1]
    assert r.stay.tolist() == [0, 1, 2]
    assert r.back.tolist() == [0, 0, 2]
    assert r.distinct_hist.tolist() == [0, 0, 5, 1]
    assert r.unique_paths.tolist() == [3, 2]
    assert r.cover.tolist() == [3, 3]
    assert r.visits.tolist() == [2, 3, 1, 1, 4, 0]
    assert r.label_pairs.tolist() == [[[5, 0], [0, 4]], [[0, 3], [0, 0]], [[1, 0], [0, 0]]]
    assert r.unlabeled.tolist() == [0, 4, 0]
    # sources given: row 0 counted from node 4 (unlabelled), row 1 from a node outside the graph
    r = walk_stats_ref.walk_stats(ids, codes, 6, labels=labels, num_classes=2, sources=[4, 6])
    assert r.label_pairs.sum() == 0 and r.unlabeled.tolist() == [9, 7, 1]
    assert r.counters.tolist() == [1, 1]            # a source is no entry of ids
    # no labels: the two label tables are absent, the rest unchanged
    r = walk_stats_ref.walk_stats(ids, codes, 6)
    assert r.label_pairs is None and r.unlabeled is None and r.step_code[2].tolist() == [2, 3, 1]


@functools.lru_cache(None)
def golden_stats(name):
    g = golden(name)
    return g, walk_stats_ref.walk_stats(g["ids"], g["codes"], int(g["n"]))


def test_restatement_on_the_cornell_golden():
    g, r = golden_stats("sampler_cornell_40_4.npz")
    assert g["ids"].reshape(-1, 40, 4).shape[0] == 366
    assert r.step_code.tolist() == [[14640, 0, 0, 0], [2614, 12026, 0, 0], [1084, 3981, 9575, 0],
                                    [436, 5996, 5254, 2954]]
    assert r.stay.sum() == 6347
    assert r.unique_paths.min() == 8
    assert r.cover.min() == 4
    assert r.cover.max() == 56
    assert r.counters.tolist() == [0, 0]


@pytest.mark.parametrize("name", golden_files("sampler_*.npz"))
def test_invariants_on_every_sampler_golden(name):
    g, r = golden_stats(name)
    W, L = int(g["W"]), int(g["L"])
    rows = g["ids"].size // (W * L)
    assert (r.step_code.sum(axis=1) == rows * W).all()
    assert all(r.step_code[t][d] == 0 for t in range(L) for d in range(L) if d > t)
    assert r.distinct_hist.sum() == rows * W and r.distinct_hist[0] == 0
    assert r.visits.sum() == rows * W * (L - 1)
    assert r.unique_paths.min() >= 1 and r.unique_paths.max() <= W
    assert r.cover.max() <= W * (L - 1) + 1
