"""CPU-side checks of the path-pattern census (pn_census.hip, pathnet_amd.synth): the goldens recorded from the reference
programs obey the recurrence the kernels implement, the new symbols are declared, exported and bound without an ABI bump,
and limits and bad arguments are refused before a device is needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import census_ref
from conftest import ROOT, golden
from pathnet_amd import _lib, synth

NEW = ("pn_census_lists_workspace_bytes", "pn_census_lists", "pn_pattern_census_workspace_bytes", "pn_pattern_census")
GOLDENS = ("census_small.npz", "census_cora.npz", "census_citeseer.npz")
FAKE = ctypes.c_void_p(4096)      # a non-null pointer that is never followed: every call below fails before any launch


@pytest.mark.parametrize("name", GOLDENS)
def test_recurrence_reproduces_the_reference_labels(name):
    g = golden(name)
    n = int(g["n"])
    assert g["u"].dtype == np.int32 and g["v"].dtype == np.int32 and g["labels"].shape == (n,)
    C = census_ref.counts_numpy(n, g["u"], g["v"], 3)
    assert C.shape == (n, 8) and C.sum() > 0
    assert (C.sum(1) < 2 ** 31).all()                   # the reference's int counters did not wrap on this input
    assert (census_ref.labels_of(C) == g["labels"]).all()
    ties = int(((C == C.max(1, keepdims=True)).sum(1) > 1).sum())
    assert ties > 0, "the golden does not exercise the tie rule"
    assert (census_ref.counts_sparse(n, g["u"], g["v"], 3) == C).all()


def test_small_golden_has_the_special_rows():
    g = golden("census_small.npz")
    n, u, v = int(g["n"]), g["u"], g["v"]
    assert n % 2 == 1 and (u == v).any()
    pairs = set()
    assert any((a, b) in pairs or pairs.add((a, b)) for a, b in zip(u.tolist(), v.tolist())), "no repeated row"
    isolated = np.setdiff1d(np.arange(n), np.concatenate([u, v]))
    assert len(isolated) > 0 and (g["labels"][isolated] == 0).all()
    # a row u == u adds two entries to that node's list
    own, _ = census_ref.entries(u, v)
    a = int(u[u == v][0])
    assert (own == a).sum() == (u == a).sum() + (v == a).sum()


def test_census_symbols_are_declared_exported_and_bound_at_abi_12():
    txt = open(os.path.join(ROOT, "include", "pathnet_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
        proto = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, code, re.S)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    declared = int(re.search(r"#define PN_ABI_VERSION (\d+)", txt).group(1))
    assert lib.pn_abi_version() == declared == _lib.ABI_VERSION == 12
    assert re.search(r"without an ABI bump", txt[txt.index("pn_census.hip"):txt.index("pn_census_lists_workspace_bytes")])


def test_workspace_sizes_need_no_device():
    lib = _lib.load()
    b = ctypes.c_int64(-1)
    _lib.check(lib.pn_census_lists_workspace_bytes(1000, 5000, ctypes.byref(b)))
    assert b.value >= 3 * 2 * 5000 * 4
    _lib.check(lib.pn_census_lists_workspace_bytes(0, 0, ctypes.byref(b)))
    assert b.value > 0
    # two level tables of n * B^(k-1) int64 counts
    for n, B, k in ((1000, 2, 3), (1000, 3, 4), (10_000_000, 2, 3), (7, 16, 2), (5, 2, 10)):
        _lib.check(lib.pn_pattern_census_workspace_bytes(n, B, k, ctypes.byref(b)))
        table = n * B ** (k - 1) * 8
        assert 2 * table <= b.value <= 2 * table + 1024, (n, B, k, b.value)
    _lib.check(lib.pn_pattern_census_workspace_bytes(1000, 2, 1, ctypes.byref(b)))
    assert 0 < b.value <= 1024


@pytest.mark.parametrize("B,k,ok", [(2, 0, False), (2, -1, False), (1, 3, False), (17, 1, False), (2, 10, True),
                                    (2, 11, False), (3, 6, True), (3, 7, False), (16, 2, True), (16, 3, False),
                                    (2, 1, True), (2, 3, True)])
def test_limits_are_checked_on_the_host(B, k, ok):
    lib = _lib.load()
    b = ctypes.c_int64(0)
    rc = lib.pn_pattern_census_workspace_bytes(100, B, k, ctypes.byref(b))
    big = 1 << 40
    rc2 = lib.pn_pattern_census(None, 0, FAKE, FAKE, None, B, k, FAKE, FAKE, FAKE, big, None)      # n = 0: no launch
    if ok:
        assert rc == _lib.PN_OK and rc2 == _lib.PN_OK
        synth.check_limits(k, B, 2)
    else:
        assert rc == _lib.PN_ERR_ARG and rc2 == _lib.PN_ERR_ARG
        assert lib.pn_last_error()
        with pytest.raises(ValueError):
            synth.check_limits(k, B, 2)


def test_counts_that_could_leave_int64_are_refused():
    synth.check_limits(3, 2, 2 ** 20)                   # 2^60
    with pytest.raises(ValueError, match="int64"):
        synth.check_limits(3, 2, 2 ** 21)               # 2^63
    with pytest.raises(ValueError, match="int64"):
        synth.check_limits(7, 2, 2 ** 9)


@pytest.mark.parametrize("case", ["no outputs", "short workspace", "no workspace", "no lists", "n<0"])
def test_bad_census_arguments_are_refused_without_a_device(case):
    lib = _lib.load()
    need = ctypes.c_int64(0)
    _lib.check(lib.pn_pattern_census_workspace_bytes(10, 2, 3, ctypes.byref(need)))
    n, off, counts, labels, ws, ws_bytes, want = 10, FAKE, FAKE, FAKE, FAKE, need.value, _lib.PN_ERR_ARG
    if case == "no outputs":
        counts = labels = None
    elif case == "short workspace":
        ws_bytes, want = need.value - 1, _lib.PN_ERR_CAPACITY
    elif case == "no workspace":
        ws, want = None, _lib.PN_ERR_CAPACITY
    elif case == "no lists":
        off = None
    elif case == "n<0":
        n = -1
    assert lib.pn_pattern_census(None, n, off, FAKE, None, 2, 3, counts, labels, ws, ws_bytes, None) == want, case
    assert lib.pn_last_error()


@pytest.mark.parametrize("case", ["n<0", "m<0", "no rows", "no off", "no adj", "too many rows", "short workspace",
                                  "no workspace"])
def test_bad_list_arguments_are_refused_without_a_device(case):
    lib = _lib.load()
    need = ctypes.c_int64(0)
    _lib.check(lib.pn_census_lists_workspace_bytes(10, 20, ctypes.byref(need)))
    n, m, u, off, adj, ws, ws_bytes, want = 10, 20, FAKE, FAKE, FAKE, FAKE, need.value, _lib.PN_ERR_ARG
    if case == "n<0":
        n = -1
    elif case == "m<0":
        m = -1
    elif case == "no rows":
        u = None
    elif case == "no off":
        off = None
    elif case == "no adj":
        adj = None
    elif case == "too many rows":
        m, ws_bytes = 1 << 30, 1 << 50
    elif case == "short workspace":
        ws_bytes, want = need.value - 1, _lib.PN_ERR_CAPACITY
    elif case == "no workspace":
        ws, want = None, _lib.PN_ERR_CAPACITY
    assert lib.pn_census_lists(None, n, m, u, FAKE, off, adj, ws, ws_bytes, None) == want, case
    assert lib.pn_last_error()
    b = ctypes.c_int64(0)
    assert lib.pn_census_lists_workspace_bytes(-1, 0, ctypes.byref(b)) == _lib.PN_ERR_ARG
    assert lib.pn_census_lists_workspace_bytes(1, 1, None) == _lib.PN_ERR_ARG


def test_cpu_device_is_refused():
    u = np.array([0, 1], np.int32)
    v = np.array([1, 2], np.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        synth.PatternCensus(3, u, v, device="cpu")
    import pathnet_amd
    assert pathnet_amd.PatternCensus is synth.PatternCensus


@pytest.mark.parametrize("argv", [[], ["cora", "citeseer"], ["--walk-len", "3"], ["--help"]])
def test_cli_wrong_argc_prints_usage(argv, capsys):
    assert synth.main(argv) == 2
    err = capsys.readouterr().err
    assert "usage: python -m pathnet_amd.synth <data_name>" in err and "--walk-len" in err
