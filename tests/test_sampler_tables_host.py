"""CPU-side checks of the device table builders' interface (pn_tables.hip): declared, bound, sized without a device,
and MerwSampler refuses an unknown build before it touches the device."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from pathnet_amd import _lib, sampler

NEW = ("pn_tables_workspace_bytes", "pn_alias_build_device", "pn_csr_build_device", "pn_hops_dense_device")


def test_device_table_builders_are_declared_and_bound():
    txt = open(os.path.join(ROOT, "include", "pathnet_hip.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert _lib.ABI_VERSION >= 11


def ws_bytes(n, m):
    b = ctypes.c_int64(-1)
    _lib.check(_lib.load().pn_tables_workspace_bytes(n, m, ctypes.byref(b)))
    return b.value


def test_tables_workspace_bytes_needs_no_device_and_is_monotone():
    assert ws_bytes(0, 0) > 0
    sizes = [(0, 0), (1, 0), (1, 1), (100, 1000), (19717, 88648), (2_000_000, 32_000_000), (10_000_000, 170_000_000)]
    got = [ws_bytes(n, m) for n, m in sizes]
    assert got == sorted(got)
    for n, m in sizes:
        assert ws_bytes(n, m) <= ws_bytes(n + 1, m) <= ws_bytes(n + 1, m + 1)
    # the caller can hold at least the sort's buffers and the alias queues
    assert ws_bytes(1000, 10 ** 6) >= 10 ** 6 * (4 * 5 + 8 * 2)
    with pytest.raises(_lib.PnError) as e:
        _lib.check(_lib.load().pn_tables_workspace_bytes(-1, 0, ctypes.byref(ctypes.c_int64())))
    assert e.value.code == _lib.PN_ERR_ARG


def test_device_entry_points_reject_bad_arguments_before_any_launch():
    lib = _lib.load()
    t = ctypes.c_int64()
    # seq_len outside 1..254, and the sort's row limit: refused before a device is needed
    for L in (0, 255):
        assert lib.pn_hops_dense_device(4, None, None, L, None, None) == _lib.PN_ERR_ARG
    assert lib.pn_alias_build_device(4, 1 << 31, None, None, None, None, None, None, None, 0, ctypes.byref(t), None, 0,
                                     None) == _lib.PN_ERR_ARG
    assert lib.pn_csr_build_device(4, 1 << 31, None, None, 0, None, None, 0, ctypes.byref(t), None, 0,
                                   None) == _lib.PN_ERR_ARG


def test_merw_sampler_rejects_unknown_build_and_hops():
    u = np.array([0, 1], np.int32)
    v = np.array([1, 0], np.int32)
    p = np.ones(2)
    with pytest.raises(ValueError, match="build"):
        sampler.MerwSampler(2, u, v, p, 4, device="cuda", build="bogus")
    with pytest.raises(ValueError, match="hops"):
        sampler.MerwSampler(2, u, v, p, 4, device="cuda", hops="sparse", build="device")
    with pytest.raises(ValueError, match="path lengths"):
        sampler.MerwSampler(2, u, v, p, 9, device="cuda:0", hops="otf", build="device")
