"""CPU-side checks of the path annotator's interface (pn_codes.hip): declared, exported and bound without an ABI bump,
sized without a device, and bad arguments refused before a device is needed."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from pathnet_amd import _lib, sampler

NEW = ("pn_path_codes_workspace_bytes", "pn_path_codes")
FAKE = ctypes.c_void_p(4096)      # a non-null pointer that is never followed: every call below fails before any launch


def tables(n=10, dense=True, csr=False):
    p = lambda on: FAKE.value if on else None       # noqa: E731
    return _lib.SamplerTables(n, 0, None, None, p(dense), p(csr), p(csr), p(csr), p(csr), 0, None)


def test_path_codes_symbols_are_declared_exported_and_bound_at_abi_12():
    txt = open(os.path.join(ROOT, "include", "pathnet_hip.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    m = re.search(r"typedef struct pn_path_report \{(.*?)\} pn_path_report;", txt, re.S)
    assert m, "pn_path_report"
    fields = re.findall(r"int64_t\s+(\w+);", m.group(1))
    assert fields == ["out_of_range", "non_edges", "far", "first_bad"]
    assert tuple(fields) == sampler.PathReport._fields
    declared = int(re.search(r"#define PN_ABI_VERSION (\d+)", txt).group(1))
    assert lib.pn_abi_version() == declared == _lib.ABI_VERSION == 12
    # the binding passes as many arguments as the header declares
    for name in NEW:
        proto = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, re.sub(r"/\*.*?\*/", "", txt, flags=re.S), re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_workspace_bytes_needs_no_device():
    lib = _lib.load()
    for tb, L in ((tables(), 4), (tables(dense=False, csr=True), 8), (tables(100000), 200)):
        b = ctypes.c_int64(-1)
        _lib.check(lib.pn_path_codes_workspace_bytes(ctypes.byref(tb), 40, L, 1000, ctypes.byref(b)))
        assert 0 < b.value <= 1 << 20
    b = ctypes.c_int64(-1)
    _lib.check(lib.pn_path_codes_workspace_bytes(ctypes.byref(tables()), 40, 4, 0, ctypes.byref(b)))     # no rows is fine
    assert b.value > 0


@pytest.mark.parametrize("case", ["rows<0", "L<1", "W<1", "otf L>8", "no hop source", "half a CSR", "null tables",
                                  "short workspace", "no workspace"])
def test_bad_arguments_are_refused_without_a_device(case):
    lib = _lib.load()
    need = ctypes.c_int64(0)
    _lib.check(lib.pn_path_codes_workspace_bytes(ctypes.byref(tables()), 5, 4, 3, ctypes.byref(need)))
    tb, W, L, rows, ws, ws_bytes = tables(), 5, 4, 3, FAKE, need.value
    if case == "rows<0":
        rows = -1
    elif case == "L<1":
        L = 0
    elif case == "W<1":
        W = 0
    elif case == "otf L>8":
        tb, L = tables(dense=False, csr=True), 9
    elif case == "no hop source":
        tb = tables(dense=False, csr=False)
    elif case == "half a CSR":
        tb = tables(dense=False, csr=True)
        tb.radj = None
    elif case == "short workspace":
        ws_bytes = need.value - 1
    elif case == "no workspace":
        ws = None
    tbp = None if case == "null tables" else ctypes.byref(tb)
    rc = lib.pn_path_codes(None, tbp, W, L, rows, FAKE, None, FAKE, None, ws, ws_bytes, None)
    assert rc == _lib.PN_ERR_ARG, (case, rc)
    assert lib.pn_last_error()
    if case not in ("short workspace", "no workspace"):
        b = ctypes.c_int64(0)
        assert lib.pn_path_codes_workspace_bytes(tbp, W, L, rows, ctypes.byref(b)) == _lib.PN_ERR_ARG, case
    # the dense table has no such limit on L
    if case == "otf L>8":
        b = ctypes.c_int64(0)
        assert lib.pn_path_codes_workspace_bytes(ctypes.byref(tables()), W, L, rows, ctypes.byref(b)) == _lib.PN_OK


def test_path_annotator_rejects_unknown_modes_before_it_touches_the_device():
    u = np.array([0, 1], np.int32)
    v = np.array([1, 0], np.int32)
    with pytest.raises(ValueError, match="build"):
        sampler.PathAnnotator(2, u, v, 4, device="cuda", build="bogus")
    with pytest.raises(ValueError, match="hops"):
        sampler.PathAnnotator(2, u, v, 4, device="cuda", hops="sparse")
    with pytest.raises(ValueError, match="path lengths"):
        sampler.PathAnnotator(2, u, v, 9, device="cuda:0", hops="otf")
