"""CPU-side checks of the path likelihoods (pn_prob.hip, pathnet_amd/pathprob.py): the interface is declared, exported and
bound without an ABI bump, sized without a device, and refuses bad arguments before a device is needed; the integer
reference the GPU tests compare against (path_prob_ref.py) sums to 2^62 for every node of three goldens; and the fp64
formulas, which are plain torch, are held to exact fractions on CPU tensors."""
import ctypes
import functools
import math
import os
import random
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import biased_ref
import path_prob_ref as ref
from conftest import ROOT, golden
from pathnet_amd import _lib, pathprob

NEW = ("pn_path_prob_workspace_bytes", "pn_path_prob")
FAKE = ctypes.c_void_p(4096)      # a non-null pointer that is never followed: every call below fails before any launch
INF = math.inf
TWO32, TWO62 = 2 ** 32, 2 ** 62
BOUND = 1e-11                     # 63 * ln(2^94) * 4 eps = 3.6e-12, rounded up


def tables(n=10, dense=True, csr=False):
    p = lambda on: FAKE.value if on else None       # noqa: E731
    return _lib.SamplerTables(n, 40, FAKE.value, FAKE.value, p(dense), p(csr), p(csr), p(csr), p(csr), 0, None)


def test_path_prob_symbols_are_declared_exported_and_bound_at_abi_12():
    txt = open(os.path.join(ROOT, "include", "pathnet_hip.h")).read()
    lib = _lib.load()
    bare = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
        proto = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, bare, re.S)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    m = re.search(r"typedef struct pn_path_prob_out \{(.*?)\} pn_path_prob_out;", bare, re.S)
    assert m, "pn_path_prob_out"
    fields = re.findall(r"(?:int64|uint8)_t\s*\*\s*(\w+);", m.group(1))
    assert tuple(fields) == _lib.PathProbOut.FIELDS == ("num", "mass", "cls", "counters")
    assert ctypes.sizeof(_lib.PathProbOut) == 8 * len(fields)
    declared = int(re.search(r"#define PN_ABI_VERSION (\d+)", txt).group(1))
    assert lib.pn_abi_version() == declared == _lib.ABI_VERSION == 12
    import pathnet_amd
    assert pathnet_amd.PathProb is pathprob.PathProb and pathnet_amd.importance_weights is pathprob.importance_weights
    assert callable(pathnet_amd.MerwSampler.path_prob) and callable(pathnet_amd.BiasedSampler.path_prob)
    assert pathprob.TRIALS == biased_ref.MAX_TRIALS


def test_workspace_query_needs_no_device():
    lib = _lib.load()
    for tb, W, L, rows, second in ((tables(), 40, 4, 366, 0), (tables(), 1, 1, 0, 1), (tables(dense=False, csr=True), 7, 6, 5, 1),
                                   (tables(dense=False), 400000, 3, 1, 0), (tables(), 40, 4, 1 << 40, 1)):
        b = ctypes.c_int64(-1)
        _lib.check(lib.pn_path_prob_workspace_bytes(ctypes.byref(tb), W, L, rows, second, ctypes.byref(b)))
        assert b.value == 0               # a transition is summed in registers: nothing is kept between launches
    assert lib.pn_path_prob_workspace_bytes(ctypes.byref(tables()), 4, 4, 1, 0, None) == _lib.PN_ERR_ARG


CASES = ["null tables", "null ids", "null out", "W<1", "L<1", "rows<0", "n<1", "no hop source", "half a CSR",
         "mass without second_order", "cls without second_order", "null triples", "neither off nor node_ref",
         "negative workspace"]


@pytest.mark.parametrize("case", CASES)
def test_bad_arguments_are_refused_without_a_device(case):
    """The query answers 0 for every shape today, so "a short or missing workspace when the query asks for one" has no
    instance yet; a negative size is the workspace error that exists."""
    lib = _lib.load()
    tb, W, L, rows, second, ids, ws_bytes = tables(), 5, 4, 3, 1, FAKE, 0
    out = _lib.PathProbOut(*([FAKE.value] * 4))
    outp = ctypes.byref(out)
    in_query = case in ("null tables", "W<1", "L<1", "rows<0", "n<1", "no hop source", "half a CSR")
    if case == "null ids":
        ids = None
    elif case == "null out":
        outp = None
    elif case == "W<1":
        W = 0
    elif case == "L<1":
        L = 0
    elif case == "rows<0":
        rows = -1
    elif case == "n<1":
        tb = tables(n=0)
    elif case == "no hop source":
        tb = tables(dense=False, csr=False)
    elif case == "half a CSR":
        tb = tables(dense=False, csr=True)
        tb.radj = None
    elif case == "mass without second_order":
        second, out.cls = 0, None
    elif case == "cls without second_order":
        second, out.mass = 0, None
    elif case == "null triples":
        tb.triples = None
    elif case == "neither off nor node_ref":
        tb.off = None
    elif case == "negative workspace":
        ws_bytes = -1
    tbp = None if case == "null tables" else ctypes.byref(tb)
    rc = lib.pn_path_prob(None, tbp, W, L, rows, ids, second, outp, None, ws_bytes, None)
    assert rc == _lib.PN_ERR_ARG, (case, rc)
    assert lib.pn_last_error()
    b = ctypes.c_int64(0)
    want = _lib.PN_ERR_ARG if in_query else _lib.PN_OK
    assert lib.pn_path_prob_workspace_bytes(tbp, W, L, rows, second, ctypes.byref(b)) == want, case


def test_first_order_needs_no_hop_source():
    """without second_order the call reads the walker table alone: the same arguments pass the query"""
    b = ctypes.c_int64(-1)
    _lib.check(_lib.load().pn_path_prob_workspace_bytes(ctypes.byref(tables(dense=False, csr=False)), 5, 4, 3, 0,
                                                        ctypes.byref(b)))
    assert b.value == 0


def test_python_surface_refuses_bad_calls_before_it_touches_the_device():
    from pathnet_amd import sampler
    view = sampler.BiasedSampler(object(), 2, .5)           # (no tables behind it: nothing below may reach for them)
    with pytest.raises(ValueError, match="kind"):
        view.path_prob(np.zeros((2, 3, 4), np.int32), kind="exact")
    nobody = type("S", (), {"device": "cpu"})()
    with pytest.raises(ValueError, match=r"\[\.\.\., W, L\]"):
        pathprob.path_prob(nobody, np.zeros(4, np.int32))
    with pytest.raises(TypeError, match="integer"):
        pathprob.path_prob(nobody, np.zeros((2, 3, 4), np.float32))


# ---- the reference itself --------------------------------------------------------------------------------------------

def test_count_a_at_its_edges():
    assert ref.count_a(-0.5) == 2 ** 31 and ref.count_a(0.0) == 2 ** 31 - 1         # r = 0 is not > 0
    assert ref.count_a(1.0) == 0 and ref.count_a(2.0) == 0      # r = 2^31 - 1 gives r / RAND_MAX = 1, which is not > 1
    assert ref.count_a(math.nextafter(1.0, 0.0)) == 1           # ... and is the only draw above the next smaller split
    assert ref.count_a(0.5) == 2 ** 31 - 2 ** 30    # r / RAND_MAX > 0.5 from r = 2^30 on


def cora_nsl_rows():
    tok = golden("refbin_shipped_cora_nsl.npz")["edge_file"].tobytes().split()
    n, m = int(tok[0]), int(tok[1])
    rows = np.array(tok[2:], dtype=np.float64).reshape(m, -1)
    return n, rows[:, 0].astype(np.int32), rows[:, 1].astype(np.int32), rows[:, 2]


@pytest.mark.parametrize("name", ["sampler_cornell_7_6.npz", "sampler_nba_5_4.npz", "cora_nsl"])
def test_numerators_of_every_node_sum_to_2_62(name):
    if name == "cora_nsl":
        n, u, v, p = cora_nsl_rows()
    else:
        g = golden(name)
        n, u, v, p = int(g["n"]), g["u"], g["v"], g["p"]
    tb = biased_ref.merw_tables(n, u, v, p)
    sizes = np.diff(tb["off"])
    assert (sizes > 0).any()
    for x in np.nonzero(sizes > 0)[0].tolist():
        row = ref.node_numerators(tb, x)
        assert sum(row.values()) == TWO62, x
        assert all(v >= 0 for v in row.values())
    for x in np.nonzero(sizes == 0)[0].tolist()[:5]:
        assert ref.node_numerators(tb, x) == {}


# ---- the fp64 formulas on CPU tensors against exact fractions --------------------------------------------------------

SPECIAL_T = (0, 1, TWO32 - 1, TWO32)


@functools.lru_cache(None)
def family():
    """A seeded family of (T, [(mass, cls, num)]) cases: 48 threshold triples x 250 transitions = 12 000 cases.  The
    thresholds cover 0, 1, 2^32 - 1 and 2^32 in every position beside random ones and the ones real (p, q) give; the masses
    cover (2^62 - 3, 2, 1) in every order, empty classes and random splits on every scale; alpha == 0 arises wherever all
    the mass lies on classes with T == 0."""
    rng = random.Random(20240611)
    Ts = [(a, b, c) for a in SPECIAL_T for b in (0, TWO32) for c in (1, TWO32 - 1)]
    Ts += [(0, 0, 0), (TWO32, TWO32, TWO32), (1, 1, 1), (0, TWO32, 0), (TWO32 - 1, TWO32 - 1, TWO32 - 1)]
    Ts += [biased_ref.thresholds(p, q) for p, q in ((1, 1), (4, .25), (.25, 4), (INF, 1), (1, INF), (INF, INF), (3, 7))]
    while len(Ts) < 48:
        Ts.append(tuple(rng.choice((rng.randrange(TWO32 + 1), rng.randrange(1 << rng.randrange(1, 33)),
                                    TWO32 - rng.randrange(1 << rng.randrange(1, 33)))) for _ in range(3)))
    out = []
    for T in Ts:
        cases = []
        for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
            m = [0, 0, 0]
            for c, v in zip(perm, (TWO62 - 3, 2, 1)):
                m[c] = v
            for cls in range(3):
                cases.append((tuple(m), cls, m[cls]))
                cases.append((tuple(m), cls, max(m[cls] // 2, 1) if m[cls] else 0))
        for c in range(3):                      # all the mass on one class
            m = [0, 0, 0]
            m[c] = TWO62
            cases.append((tuple(m), c, rng.randrange(1, TWO62 + 1)))
            cases.append((tuple(m), (c + 1) % 3, 0))
        while len(cases) < 250:
            scale = 1 << rng.randrange(1, 63)   # one class anywhere from a few units to most of the table
            a = rng.randrange(min(scale, TWO62) + 1)
            b = rng.randrange(min(1 << rng.randrange(1, 63), TWO62 - a) + 1)
            m = [a, b, TWO62 - a - b]
            rng.shuffle(m)
            cls = rng.randrange(3)
            num = rng.choice((m[cls], rng.randrange(m[cls] + 1), min(m[cls], rng.randrange(1, 1 << rng.randrange(1, 63)))))
            cases.append((tuple(m), cls, num))
        out.append((T, cases))
    return out


def as_tensors(cases):
    mass = torch.tensor([c[0] for c in cases], dtype=torch.int64)
    cls = torch.tensor([c[1] for c in cases], dtype=torch.uint8)
    num = torch.tensor([c[2] for c in cases], dtype=torch.int64)
    return num, mass, cls


def worst_error(got, exact):
    worst = 0.0
    for g, e in zip(got, exact):
        if e == 0:
            assert g == 0.0
        elif e >= Fraction(1e-290):
            worst = max(worst, ref.rel_err(g, e))
    return worst


def test_realised_formula_against_fractions():
    """relative error <= 1e-11 wherever the exact value is >= 1e-290, over the whole family; and the family is sharp enough
    to tell: the same formula with 1 - alpha formed by subtraction misses the bound on it"""
    worst = naive_worst = 0.0
    total = zero_alpha = 0
    for T, cases in family():
        num, mass, cls = as_tensors(cases)
        got = pathprob.realised_step(num, mass, cls, T).tolist()
        exact = [ref.realised(c[2], c[0], c[1], T) for c in cases]
        worst = max(worst, worst_error(got, exact))
        total += len(cases)
        zero_alpha += sum(1 for m, _, _ in cases if all(mc == 0 or t == 0 for mc, t in zip(m, T)))
        # the subtraction form, for the family's sharpness only
        m = mass.double() / TWO62
        a = [t / TWO32 for t in T]
        alpha = m[:, 0] * a[0] + m[:, 1] * a[1] + m[:, 2] * a[2]
        rest = (1.0 - alpha) ** 63
        naive = torch.where(alpha > 0, num.double() / TWO62 * torch.tensor(a, dtype=torch.float64)[cls.long()] *
                            (1.0 - rest) / torch.where(alpha > 0, alpha, torch.ones_like(alpha)) + rest * num.double() / TWO62,
                            num.double() / TWO62)
        naive_worst = max(naive_worst, max((ref.rel_err(g, e) for g, e in zip(naive.tolist(), exact) if e > 0), default=0.0))
    print("realised: %d cases, %d with alpha == 0, worst relative error %.3g (subtraction form %.3g)"
          % (total, zero_alpha, worst, naive_worst))
    assert total >= 10000 and zero_alpha >= 100
    assert worst <= BOUND, worst
    assert naive_worst > BOUND, naive_worst


@pytest.mark.parametrize("p,q", [(1, 1), (4, .25), (.25, 4), (INF, 1), (1, INF), (INF, INF), (3, 7)])
def test_target_formula_against_fractions(p, q):
    worst = 0.0
    for _, cases in family()[::6]:
        num, mass, cls = as_tensors(cases)
        got = pathprob.target_step(num, mass, cls, p, q).tolist()
        worst = max(worst, worst_error(got, [ref.target(c[2], c[0], c[1], p, q) for c in cases]))
    assert worst <= BOUND, worst


def test_transition_without_a_class_is_the_plain_table_step():
    num = torch.tensor([TWO62 // 3, 0, TWO62], dtype=torch.int64)
    mass = torch.zeros((3, 3), dtype=torch.int64)
    cls = torch.full((3,), 3, dtype=torch.uint8)
    want = (num.double() / TWO62).tolist()
    assert pathprob.realised_step(num, mass, cls, biased_ref.thresholds(4, .25)).tolist() == want
    assert pathprob.target_step(num, mass, cls, INF, INF).tolist() == want
    assert pathprob.table_step(num).tolist() == want


def test_logp_adds_in_step_order_and_keeps_impossible_paths_at_minus_infinity():
    step = torch.tensor([[0.5, 0.25, 0.125], [0.5, 0.0, 0.125], [1.0, 1.0, 1.0]], dtype=torch.float64)
    lp = pathprob.path_logp(step)
    assert lp[0].item() == (math.log(0.5) + math.log(0.25)) + math.log(0.125)
    assert lp[1].item() == -INF and lp[2].item() == 0.0
    assert pathprob.path_logp(torch.zeros((4, 0), dtype=torch.float64)).tolist() == [0.0] * 4     # L = 1: no step


def prob_of(logp):
    z = torch.zeros(0)
    return pathprob.PathProb(z, z, torch.tensor(logp, dtype=torch.float64), z, None, None)


def test_importance_weights_on_cpu_tensors():
    t = prob_of([[math.log(.5), math.log(.25), -INF, -INF], [-INF, -INF, -INF, -INF], [math.log(.125), 0.0, -1.0, -INF]])
    q = prob_of([[math.log(.25), math.log(.5), math.log(.5), -INF], [math.log(.5), -1.0, -2.0, -3.0], [-INF, 0.0, -1.0, -2.0]])
    w = pathprob.importance_weights(t, q, normalize=False)
    assert w[0].tolist() == [2.0, 0.5, 0.0, 0.0]            # impossible under the target: 0, whatever the proposal says
    assert w[1].tolist() == [0.0] * 4
    assert math.isnan(w[2, 0].item()) and w[2, 1:].tolist() == [1.0, 1.0, 0.0]      # impossible under the proposal alone
    wn = pathprob.importance_weights(t, q)
    assert wn[0].tolist() == [0.8, 0.2, 0.0, 0.0]
    assert wn[1].tolist() == [0.0] * 4                      # a row whose weights sum to 0 stays 0
    assert all(math.isnan(x) for x in wn[2].tolist())       # a nan weight is a nan sum: the row says so
    with pytest.raises(ValueError, match="likelihoods of"):
        pathprob.importance_weights(t, prob_of([[0.0]]))
