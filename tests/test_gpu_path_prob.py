"""GPU path likelihoods (pn_path_prob, smp.path_prob, smp.biased(p, q).path_prob, importance_weights) against the integer /
fraction reference tests/path_prob_ref.py.  Numerators, class masses, classes and counters are compared bit for bit; the
fp64 probabilities are held to exact fractions within 1e-11 (the bound derived in test_path_prob_host.py) and the
log-likelihoods to math.log sums within 1e-12 * max(1, |logp|): at most 7 terms at about 1 ulp each, with a 100x margin."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import biased_ref
import path_prob_ref as ref
from conftest import golden

pytestmark = pytest.mark.gpu

INF = math.inf
TWO62 = 2 ** 62
PQ = [(1, 1), (4, .25), (INF, 1), (1, INF), (INF, INF)]


def dev32(a):
    return torch.as_tensor(np.asarray(a, np.int32)).cuda()


def same(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: first mismatch at %s: got %s want %s" % (what, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def log_sums(num):
    """math.log of every step's exact probability, added in step order"""
    out = []
    for path in num.reshape(-1, num.shape[-1]).tolist():
        acc = 0.0
        for v in path:
            acc = acc + math.log(v / TWO62)
        out.append(acc)
    return np.array(out).reshape(num.shape[:-1])


@functools.lru_cache(None)
def case(name):
    """-> golden, reference tables, the ids under test and their reference, computed once and never written to"""
    g = golden(name)
    n, L = int(g["n"]), int(g["L"])
    ids = g["ids"]
    if name.startswith("uniform"):
        tb = biased_ref.uniform_tables(n, g["u"], g["v"])
    else:
        tb = biased_ref.merw_tables(n, g["u"], g["v"], g["p"])
    if name == "sampler_cora_40_4.npz":
        ids = ids[:, :64]                       # the first 64 source rows
    want = ref.path_prob(tb, ids, second_order=name == "sampler_cornell_7_6.npz")
    for v in want.values():
        v.setflags(write=False)
    return g, tb, ids, want


@functools.lru_cache(None)
def sampler_of(name, hops="dense"):
    from pathnet_amd import MerwSampler, UniformSampler
    g = golden(name)
    n, L = int(g["n"]), int(g["L"])
    if name.startswith("uniform"):
        return UniformSampler(n, g["u"], g["v"], L, hops=hops)
    return MerwSampler(n, g["u"], g["v"], g["p"], L, hops=hops)


CORNELL = "sampler_cornell_7_6.npz"


@pytest.mark.parametrize("name", [CORNELL, "sampler_nba_5_4.npz", "sampler_cora_40_4.npz", "uniform_ring37_5_4.npz"])
def test_goldens_bit_equal_numerators_and_finite_likelihoods(name):
    """Cornell: tables of 4..190 triples, thresholds of exactly 2^31; Nba: tables to 442 triples (more than one stride of a
    group); cora: negative and > 1 rows; the uniform ring: k = 3, so 2^31 % k != 0"""
    g, tb, ids, want = case(name)
    if name == "uniform_ring37_5_4.npz":
        assert 3 in np.diff(tb["off"])
    pp = sampler_of(name).path_prob(dev32(ids))
    assert pp.mass is None and pp.cls is None
    assert pp.num.dtype == torch.int64 and tuple(pp.num.shape) == ids.shape[:-1] + (ids.shape[-1] - 1,)
    same(pp.num, want["num"], "num")
    assert pp.counters.tolist() == [0, 0, 0, 0]
    assert (want["num"] > 0).all()
    step, logp = pp.step.cpu().numpy(), pp.logp.cpu().numpy()
    assert pp.logp.dtype == torch.float64 and logp.shape == ids.shape[:-1]
    assert np.isfinite(logp).all()
    assert (step == want["num"].astype(np.float64) / TWO62).all()
    sums = log_sums(want["num"])
    assert (np.abs(logp - sums) <= 1e-12 * np.maximum(1.0, np.abs(sums))).all(), np.abs(logp - sums).max()
    s = pp.summary()
    assert s["paths"] == s["possible_paths"] == logp.size and s["impossible"] == 0
    assert abs(s["mean_logp"] - sums.mean()) <= 1e-12 * abs(sums.mean())


# ---- hand-built tables -----------------------------------------------------------------------------------------------

SIZES = (1, 2, 3, 15, 16, 17, 63, 64, 65, 1000)     # node i has SIZES[i] rows: around one and four strides of a group, and a hub
N_HAND = 1013


@functools.lru_cache(None)
def hand():
    """Nodes 0..9 have SIZES[i] rows to the nodes 10, 11, ..; node 10 has four rows with a zero and a negative p; node 11 has
    two rows of p = 0.5 (both S exactly 1.0, as node 0's single row); every other node has no rows."""
    rng = np.random.default_rng(5)
    u, v, p = [], [], []
    for i, k in enumerate(SIZES):
        w = rng.random(k) + 0.05
        w = w / w.sum()
        if k == 1:
            w[:] = 1.0
        u += [i] * k
        v += list(range(10, 10 + k))
        p += w.tolist()
    u += [10] * 4 + [11] * 2
    v += [0, 1, 2, 3, 4, 5]
    p += [0.7, 0.0, -0.1, 0.4, 0.5, 0.5]
    u, v, p = np.array(u, np.int32), np.array(v, np.int32), np.array(p)
    tb = biased_ref.merw_tables(N_HAND, u, v, p)
    assert (tb["S"] == 1.0).sum() >= 3 and (np.diff(tb["off"])[:10] == SIZES).all() and np.diff(tb["off"])[12:].max() == 0
    from pathnet_amd import MerwSampler
    return tb, MerwSampler(N_HAND, u, v, p, 4)


def test_hand_built_tables_every_transition_of_every_size():
    """every (node, target) pair of the hand-built tables as an L = 2 path, a non-neighbour per node beside them"""
    tb, smp = hand()
    pairs = []
    for i, k in enumerate(SIZES):
        pairs += [(i, x) for x in range(10, 10 + k)] + [(i, 10 + k)]         # the last one is no neighbour
    pairs += [(10, x) for x in range(0, 5)] + [(11, 4), (11, 5), (11, 6)]
    ids = np.array(pairs, np.int32).reshape(1, -1, 2)
    want = ref.path_prob(tb, ids)
    pp = smp.path_prob(dev32(ids))
    same(pp.num, want["num"], "num")
    assert pp.counters.tolist() == want["counters"].tolist()
    assert want["counters"][2] >= len(SIZES) + 1 and want["counters"][0] == want["counters"][1] == 0
    # per node the numerators of its neighbours sum to 2^62 exactly
    sums = torch.zeros(N_HAND, dtype=torch.int64, device="cuda").index_add_(0, dev32(ids[0, :, 0]).long(), pp.num.reshape(-1))
    assert sums[:12].tolist() == [TWO62] * 12
    imp = pp.num.reshape(-1) == 0
    assert torch.isinf(pp.logp.reshape(-1)[imp]).all() and torch.isfinite(pp.logp.reshape(-1)[~imp]).all()


def test_caller_paths_impossible_empty_and_out_of_range():
    tb, smp = hand()
    n = N_HAND
    ids = np.array([[[9, 500, 501, 3],        # hub -> 500, then out of an empty table twice
                     [2, 11, 4, 20],          # a possible path: 2 -> 11 -> 4 -> 20
                     [2, 13, 2, 10],          # 2 -> 13 is no row (impossible), 13 has no rows, 2 -> 10 is one
                     [-1, 3, n, n],           # ids outside the graph: transitions with one, one and two of them
                     [3, 10, -1, 12]],        # a bad id in the middle of a path is seen by both its transitions
                    [[0, 10, 0, 10]] * 5], np.int32)
    want = ref.path_prob(tb, ids)
    assert want["counters"].tolist() == [6, 3, 1, 0]
    pp = smp.path_prob(dev32(ids))
    same(pp.num, want["num"], "num")
    assert pp.counters.tolist() == want["counters"].tolist()
    logp = pp.logp.cpu().numpy()
    assert np.isfinite(logp[0, 1]) and np.isfinite(logp[1]).all()
    assert (logp[0, [0, 2, 3, 4]] == -INF).all()
    s = pp.summary()
    assert (s["bad_ids"], s["empty_tables"], s["impossible"], s["paths"], s["possible_paths"]) == (6, 3, 1, 10, 6)
    # second order over the same paths: a bad id or a bad prev classifies nothing
    sec = smp.biased(2, .5).path_prob(dev32(ids))
    want2 = ref.path_prob(tb, ids, second_order=True)
    same(sec.num, want2["num"], "num")
    same(sec.mass, want2["mass"], "mass")
    same(sec.cls, want2["cls"], "cls")
    assert sec.counters.tolist() == want2["counters"].tolist()
    assert want2["cls"][0, 3].tolist() == [3, 3, 3] and want2["cls"][0, 4].tolist() == [3, 3, 3]


@pytest.mark.parametrize("shape", [(3, 5, 4), (1, 1, 2), (2, 3, 1), (0, 5, 4)])
def test_shapes(shape):
    """45 transitions (no multiple of a group of 16 lanes), a single one, L = 1 and rows = 0: the last two only zero the counters"""
    tb, smp = hand()
    rng = np.random.default_rng(sum(shape))
    ids = rng.integers(0, 30, shape).astype(np.int32)          # nodes 0..29: rows, non-rows and empty tables alike
    want = ref.path_prob(tb, ids)
    pp = smp.path_prob(dev32(ids))
    assert tuple(pp.num.shape) == shape[:-1] + (shape[-1] - 1,) and tuple(pp.logp.shape) == shape[:-1]
    same(pp.num, want["num"], "num")
    assert pp.counters.tolist() == want["counters"].tolist()
    if shape[-1] == 1:
        assert pp.logp.tolist() == [[0.0] * shape[1]] * shape[0]
    sec = smp.biased(1, 1).path_prob(dev32(ids), kind="target")
    want2 = ref.path_prob(tb, ids, second_order=True)
    same(sec.mass, want2["mass"], "mass")
    same(sec.cls, want2["cls"], "cls")
    assert sec.counters.tolist() == want2["counters"].tolist()


def test_row_sums_on_the_device_are_exactly_2_62():
    g, tb, _, _ = case(CORNELL)
    n = int(g["n"])
    pairs = [(u, x) for u in range(n) for x in sorted(ref.node_numerators(tb, u))]
    ids = dev32(pairs).reshape(1, -1, 2)
    pp = sampler_of(CORNELL).path_prob(ids)
    sums = torch.zeros(n, dtype=torch.int64, device="cuda").index_add_(0, ids[0, :, 0].long(), pp.num.reshape(-1))
    assert sums.tolist() == [TWO62] * n
    assert pp.counters[:2].tolist() == [0, 0]


# ---- second order ----------------------------------------------------------------------------------------------------

def test_second_order_masses_and_classes_dense_and_otf():
    g, tb, ids, want = case(CORNELL)
    got = {}
    for hops in ("dense", "otf"):
        pp = got[hops] = sampler_of(CORNELL, hops).biased(4, .25).path_prob(dev32(ids))
        same(pp.num, want["num"], "num")
        same(pp.mass, want["mass"], "mass")
        same(pp.cls, want["cls"], "cls")
        assert pp.counters.tolist() == [0, 0, 0, 0]
        assert (pp.mass[..., 1:, :].sum(-1) == TWO62).all() and (pp.mass[..., 0, :] == 0).all()
        assert (pp.cls[..., 0] == 3).all() and (pp.cls[..., 1:] < 3).all()
    for f in ("num", "mass", "cls", "step", "logp"):
        assert torch.equal(getattr(got["dense"], f), getattr(got["otf"], f)), f
    assert set(np.unique(want["cls"])) == {0, 1, 2, 3}


@pytest.mark.parametrize("p,q", PQ)
def test_realised_and_target_probabilities_against_fractions(p, q):
    """every distinct (num, mass, cls) among the Cornell transitions, under both kinds"""
    g, tb, ids, want = case(CORNELL)
    view = sampler_of(CORNELL).biased(p, q)
    T = biased_ref.thresholds(p, q)
    assert view.thresholds == T
    num, mass, cls = want["num"].reshape(-1), want["mass"].reshape(-1, 3), want["cls"].reshape(-1)
    exact = {"realised": {}, "target": {}}
    for kind in exact:
        step = view.path_prob(dev32(ids), kind=kind).step.cpu().numpy().reshape(-1)
        worst = 0.0
        for i, key in enumerate(zip(num.tolist(), map(tuple, mass.tolist()), cls.tolist())):
            if key not in exact[kind]:
                exact[kind][key] = (ref.realised(*key, T) if kind == "realised" else ref.target(*key, p, q))
            e = exact[kind][key]
            if e == 0:
                assert step[i] == 0.0
            else:
                worst = max(worst, ref.rel_err(float(step[i]), e))
        print("%s (%s, %s): %d distinct transitions, worst relative error %.3g" % (kind, p, q, len(exact[kind]), worst))
        assert worst <= 1e-11, (kind, worst)


def test_leaf_under_p_inf_is_the_plain_table_step():
    """0 - 1 - 2, node 2 a leaf: arriving from 1 its only proposal is the return, which p = inf never accepts, so alpha = 0
    and the 64th proposal is taken: P = q_x"""
    from pathnet_amd import MerwSampler
    u = np.array([0, 1, 1, 2], np.int32)
    v = np.array([1, 0, 2, 1], np.int32)
    p = np.array([1.0, 0.5, 0.5, 1.0])
    smp = MerwSampler(3, u, v, p, 3)
    ids = dev32([[[1, 2, 1], [0, 1, 2], [0, 1, 0]]])
    for kind, want_back, want_return in (("realised", 1.0, 2.0 ** -64), ("target", 0.0, 0.0)):
        pp = smp.biased(INF, 1).path_prob(ids, kind=kind)
        assert pp.mass[0, 0, 1].tolist() == [TWO62, 0, 0] and pp.cls[0, 0].tolist() == [3, 0]
        assert pp.step[0, 0].tolist() == [0.5, want_back]
        assert pp.num[0, 0].tolist() == [TWO62 // 2, TWO62]
        # from 1, having come from 0: the return is never accepted, 2 always -- so the walker returns only when 63 trials
        # proposed the return and the 64th does too: 2^-64
        assert pp.step[0, 1].tolist() == [1.0, 1.0] and pp.step[0, 2, 0].item() == 1.0
        assert abs(pp.step[0, 2, 1].item() - want_return) <= 1e-11 * want_return


# ---- the walker agrees with its own likelihood -----------------------------------------------------------------------

@pytest.mark.parametrize("p,q,seed", [(1, 1, 12345), (4, .25, 777)])
def test_walker_frequencies_agree_with_path_prob(p, q, seed):
    """400 000 walks of three nodes from node 48 of Cornell.  The first step, and the second step given every first-step
    node reached at least 3 000 times, are multinomial draws with the cell probabilities path_prob gives, so every cell
    with 0 < P < 1 must hold |count - m P| <= 5 sqrt(m P (1 - P)), and no node outside the support may occur.  The outcome
    is deterministic; the CPU restatement of the same draws (tests/biased_ref.py) with the fractions of path_prob_ref.py
    gave, over the 95 first-step and 409 second-step cells of each run, a worst z of 2.70 and 2.77 for (1, 1) and of 3.00
    and 3.64 for (4, .25), which had 320 exhausted steps."""
    from pathnet_amd import MerwSampler
    g, tb, _, _ = case(CORNELL)
    n, src, m = int(g["n"]), 48, 400000
    smp = MerwSampler(n, g["u"], g["v"], g["p"], 3, hops="dense")
    view = smp.biased(p, q)
    ids, _ = view.sample(m, seed, nodes=dev32([src]))
    walks = ids.reshape(m, 3).cpu().numpy().astype(np.int64)
    assert (walks[:, 0] == src).all()
    first = np.bincount(walks[:, 1], minlength=n)
    firsts = [c for c in range(n) if first[c] >= 3000]
    assert len(firsts) >= 5
    # the queries: (src, x, x) for every node x -- only its first step is read -- and (src, c, x) for every kept c and every x
    q1 = [(src, x, x) for x in range(n)]
    q2 = [(src, c, x) for c in firsts for x in range(n)]
    pp = view.path_prob(dev32(q1 + q2).reshape(1, -1, 3))
    step = pp.step.reshape(-1, 2).cpu().numpy()
    worst = cells = 0

    def hold(counts, P, total):
        nonlocal worst, cells
        assert abs(P.sum() - 1.0) <= 1e-12
        for x in range(n):
            if P[x] == 0.0:
                assert counts[x] == 0, "node %d drawn outside the support" % x
            elif P[x] < 1.0:
                z = abs(counts[x] - total * P[x]) / math.sqrt(total * P[x] * (1.0 - P[x]))
                worst, cells = max(worst, z), cells + 1
                assert z <= 5.0, (x, counts[x], total * P[x], z)

    hold(first, step[:n, 0], m)
    assert {x for x in range(n) if step[x, 0] > 0} == {x for x, v in ref.node_numerators(tb, src).items() if v > 0}
    for k, c in enumerate(firsts):
        sel = walks[walks[:, 1] == c]
        hold(np.bincount(sel[:, 2], minlength=n), step[n + k * n:n + (k + 1) * n, 1], len(sel))
    print("(%s, %s): %d cells, worst z %.2f, %d exhausted steps" % (p, q, cells, worst, view.exhausted_steps()))
    assert cells == 95 + 409


# ---- importance weights ----------------------------------------------------------------------------------------------

def test_importance_weights_towards_the_plain_table():
    import pathnet_amd
    g, tb, _, _ = case(CORNELL)
    smp = sampler_of(CORNELL)
    view = smp.biased(4, .25)
    ids, _ = view.sample(7, 99)
    proposal = view.path_prob(ids)
    target = smp.path_prob(ids)
    assert torch.equal(proposal.num, target.num)
    w = pathnet_amd.importance_weights(target, proposal)
    assert tuple(w.shape) == (1, 183, 7) and w.dtype == torch.float64
    assert ((w.sum(-1) - 1.0).abs() <= 1e-12).all() and (w > 0).all()
    raw = pathnet_amd.importance_weights(target, proposal, normalize=False)
    assert ((raw / raw.sum(-1, keepdim=True) - w).abs() <= 1e-15).all()
    # the exact ratio for the first 24 rows
    T = biased_ref.thresholds(4, .25)
    rows = 24
    want = ref.path_prob(tb, ids[0, :rows].cpu().numpy(), second_order=True)
    got = w[0, :rows].cpu().numpy()
    worst = 0.0
    for r in range(rows):
        ratio = []
        for k in range(7):
            pt = pq = Fraction(1)
            for t in range(5):
                key = (want["num"][r, k, t], want["mass"][r, k, t], want["cls"][r, k, t])
                pt *= Fraction(int(key[0]), TWO62)
                pq *= ref.realised(*key, T)
            ratio.append(pt / pq)
        for k in range(7):
            worst = max(worst, ref.rel_err(float(got[r, k]), ratio[k] / sum(ratio)))
    assert worst <= 1e-11, worst
