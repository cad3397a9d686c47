"""CPU-side checks of the biased walker's interface (pn_bias.hip): declared, exported and bound without an ABI bump, the
thresholds against their fp64 formula, bad arguments refused before a device is needed, and the distribution the CPU
restatement (tests/biased_ref.py) realises against the exact second-order transition probabilities."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import biased_ref
from conftest import ROOT
from oracle import merw
from pathnet_amd import _lib, sampler

NEW = ("pn_bias_thresholds", "pn_sample_paths_biased_workspace_bytes", "pn_sample_paths_biased")
FAKE = ctypes.c_void_p(4096)      # a non-null pointer that is never followed: every call below fails before any launch
INF = math.inf


def tables(n=10, dense=True, csr=False):
    p = lambda on: FAKE.value if on else None       # noqa: E731
    return _lib.SamplerTables(n, 40, FAKE.value, FAKE.value, p(dense), p(csr), p(csr), p(csr), p(csr), 0, None)


def test_bias_symbols_are_declared_exported_and_bound_at_abi_12():
    txt = open(os.path.join(ROOT, "include", "pathnet_hip.h")).read()
    lib = _lib.load()
    bare = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
        proto = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, bare, re.S)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert int(re.search(r"#define PN_BIAS_MAX_TRIALS (\d+)", txt).group(1)) == biased_ref.MAX_TRIALS == 64
    declared = int(re.search(r"#define PN_ABI_VERSION (\d+)", txt).group(1))
    assert lib.pn_abi_version() == declared == _lib.ABI_VERSION == 12
    import pathnet_amd
    assert pathnet_amd.BiasedSampler is sampler.BiasedSampler


@pytest.mark.parametrize("p,q", [(1, 1), (4, .25), (.25, 4), (INF, 1), (INF, .5), (3, 7)])
def test_thresholds_equal_the_fp64_formula(p, q):
    w = [0.0 if math.isinf(p) else 1.0 / p, 1.0, 0.0 if math.isinf(q) else 1.0 / q]
    want = tuple(int(math.floor(math.ldexp(x / max(w), 32))) for x in w)
    got = sampler.bias_thresholds(p, q)
    assert got == want == biased_ref.thresholds(p, q)
    assert max(got) == 2 ** 32 and min(got) >= 0            # the largest class is always accepted
    assert got[w.index(max(w))] == 2 ** 32


@pytest.mark.parametrize("p,q", [(0, 1), (1, 0), (-1, 1), (1, -2.5), (math.nan, 1), (1, math.nan), (-INF, 1)])
def test_thresholds_refuse_zero_negative_and_nan(p, q):
    thr = (ctypes.c_uint64 * 3)()
    lib = _lib.load()
    assert lib.pn_bias_thresholds(float(p), float(q), thr) == _lib.PN_ERR_ARG
    assert lib.pn_last_error()
    with pytest.raises(ValueError):
        sampler.bias_thresholds(p, q)
    with pytest.raises(ValueError):
        sampler.BiasedSampler(object(), p, q)       # the view refuses them when it is made, without a device


def test_workspace_query_needs_no_device():
    lib = _lib.load()
    b = ctypes.c_int64(-1)
    _lib.check(lib.pn_sample_paths_biased_workspace_bytes(ctypes.byref(tables()), 40, 4, 2, 1000, ctypes.byref(b)))
    assert b.value == 0                                     # dense: the walker reads the code bytes itself
    _lib.check(lib.pn_sample_paths_biased_workspace_bytes(ctypes.byref(tables(dense=False, csr=True)), 40, 8, 2, 1000,
                                                          ctypes.byref(b)))
    c = ctypes.c_int64(-1)
    _lib.check(lib.pn_path_codes_workspace_bytes(ctypes.byref(tables(dense=False, csr=True)), 40, 8, 2000, ctypes.byref(c)))
    assert b.value == c.value > 0                           # on the fly: what the code launch needs
    _lib.check(lib.pn_sample_paths_biased_workspace_bytes(ctypes.byref(tables()), 40, 4, 0, 0, ctypes.byref(b)))   # empty window


@pytest.mark.parametrize("case", ["null tables", "W<1", "L<1", "no hop source", "half a CSR", "otf L>8", "p=0", "q<0",
                                  "p nan", "short workspace", "no workspace", "null ids", "window past n"])
def test_bad_arguments_are_refused_without_a_device(case):
    lib = _lib.load()
    otf = tables(dense=False, csr=True)
    need = ctypes.c_int64(0)
    _lib.check(lib.pn_sample_paths_biased_workspace_bytes(ctypes.byref(otf), 5, 4, 1, 3, ctypes.byref(need)))
    assert need.value > 0
    tb, W, L, p, q, ids, ws, ws_bytes, count = tables(), 5, 4, 2.0, 0.5, FAKE, FAKE, need.value, 3
    if case == "W<1":
        W = 0
    elif case == "L<1":
        L = 0
    elif case == "no hop source":
        tb = tables(dense=False, csr=False)
    elif case == "half a CSR":
        tb = tables(dense=False, csr=True)
        tb.radj = None
    elif case == "otf L>8":
        tb, L = otf, 9
    elif case == "p=0":
        p = 0.0
    elif case == "q<0":
        q = -1.0
    elif case == "p nan":
        p = math.nan
    elif case == "short workspace":
        tb, ws_bytes = otf, need.value - 1
    elif case == "no workspace":
        tb, ws = otf, None
    elif case == "null ids":
        ids = None
    elif case == "window past n":
        count = 11
    tbp = None if case == "null tables" else ctypes.byref(tb)
    rc = lib.pn_sample_paths_biased(None, tbp, W, L, 1, 0, 1, 0, count, p, q, ids, FAKE, None, ws, ws_bytes, None, None,
                                    None, None)
    assert rc == _lib.PN_ERR_ARG, (case, rc)
    assert lib.pn_last_error()
    if case in ("null tables", "W<1", "L<1", "no hop source", "half a CSR", "otf L>8"):
        b = ctypes.c_int64(0)
        assert lib.pn_sample_paths_biased_workspace_bytes(tbp, W, L, 1, count, ctypes.byref(b)) == _lib.PN_ERR_ARG, case


def test_view_refuses_the_glibc_replay_before_it_touches_the_device():
    view = sampler.BiasedSampler(object(), 2, .5)           # (no tables behind it: nothing below may reach for them)
    with pytest.raises(ValueError, match="Philox"):
        view.sample(4, 1, draw_source=sampler.DRAW_GLIBC_REPLAY)
    assert view.exhausted_steps() == 0
    assert view.thresholds == biased_ref.thresholds(2, .5)


def test_cli_bias_without_philox_exits_with_status_2(tmp_path):
    r = subprocess.run([sys.executable, "-m", "pathnet_amd.sampler", "g", "3", "4", "--bias", "2,0.5", "--in",
                        os.path.join(tmp_path, "absent.in"), "--out-root", str(tmp_path) + "/"], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 2, (r.returncode, r.stderr[-300:])
    assert "--draw philox" in r.stderr
    assert not os.listdir(tmp_path)


def test_vectorised_philox_equals_the_oracle():
    rng = np.random.default_rng(3)
    for seed in (0, 77, 0xC0FFEE1234, 2 ** 64 - 1):
        sub = rng.integers(0, 2 ** 63, 6, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        ctr = np.array([0, 1, 2, 63, 64, 2 ** 31], np.uint64)
        w = biased_ref.philox_blocks(seed, sub, ctr)
        for i in range(6):
            for k in range(4):
                assert int(w[k, i]) == merw.philox_draw(seed, int(sub[i]), 4 * int(ctr[i]) + k)


def test_restatement_realises_the_second_order_distribution():
    """(p, q) = (2, 0.5) over uniform tables on a 6-node graph: a triangle 0-1-2, a tail 2-3-4 with the chord 1-4 and the
    pendant node 5 on 4; build_uniform adds every node's self loop.  For every state (prev, cur) with at least one visit
    the frequency f of each next node x is compared with the exact pi = P_table(cur -> x) a(prev, x) / Z.
    Bound: the N visits of a state draw x independently with probability pi (rejection sampling is exact while no step
    comes to the cap -- asserted), so f is binomial with standard deviation sqrt(pi (1 - pi) / N); five of them leave
    each of the ~70 comparisons a failure probability under 6e-7.  Nothing here is tuned: the seed is the only choice, and
    the run is deterministic."""
    p, q = 2.0, 0.5
    u = np.array([0, 1, 0, 2, 3, 1, 4], np.int32)
    v = np.array([1, 2, 2, 3, 4, 4, 5], np.int32)
    n, W, L = 6, 7000, 41
    tb = biased_ref.uniform_tables(n, u, v)
    res = biased_ref.walk(tb, W, L, 20240517, p, q, codes=False)
    assert res.exhausted == 0               # the cap must not be what makes this pass
    assert not res.empty and res.steps == n * W * (L - 1)
    ids = res.ids.reshape(-1, L).astype(np.int64)
    edges = set(zip(tb["eu"].tolist(), tb["ev"].tolist()))
    out = {a: tb["A"][tb["off"][a]:tb["off"][a + 1]].tolist() for a in range(n)}
    prev, cur, nxt = ids[:, :-2].ravel(), ids[:, 1:-1].ravel(), ids[:, 2:].ravel()
    counts = np.zeros((n, n, n), np.int64)
    np.add.at(counts, (prev, cur, nxt), 1)
    states = [(a, b) for a in range(n) for b in out[a]]          # every (prev, cur) a walk can be in, self loops included
    assert len(states) == len(edges) == 2 * len(u) + n
    checked = 0
    for a, b in states:
        N = int(counts[a, b].sum())
        assert N >= 20000, ((a, b), N)
        weight = {}
        for x in out[b]:                # uniform table: every listed neighbour has P_table = 1 / len
            alpha = 1.0 / p if x == a else (1.0 if (a, x) in edges else 1.0 / q)
            weight[x] = weight.get(x, 0.0) + alpha / len(out[b])
        Z = sum(weight.values())
        assert counts[a, b].sum() == sum(counts[a, b, x] for x in weight)     # nothing outside cur's list
        for x, wx in weight.items():
            pi = wx / Z
            f = counts[a, b, x] / N
            assert abs(f - pi) <= 5.0 * math.sqrt(pi * (1.0 - pi) / N), ((a, b, x), f, pi, N)
            checked += 1
    assert checked >= 60
    # and the first step is the plain table step
    first = np.zeros((n, n), np.int64)
    np.add.at(first, (ids[:, 0], ids[:, 1]), 1)
    for a in range(n):
        for x in out[a]:
            pi = 1.0 / len(out[a])
            assert abs(first[a, x] / W - pi) <= 5.0 * math.sqrt(pi * (1.0 - pi) / W)
