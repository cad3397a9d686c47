"""tests/cluster_ref.py on the CPU: the score restatement against scikit-learn, the checkers against every named wrong
implementation, the decidability of the blob trajectories the GPU test compares label for label, and the parts of
pn_kmeans_* that need no device (workspace formula, plan, refusals)."""
import ctypes

import numpy as np
import pytest

import cluster_ref as ref


# ---- scores ---------------------------------------------------------------------------------------------------------------------
def random_labels(i):
    rng = np.random.default_rng(1000 + i)
    n = int(rng.integers(2, 401))
    K = 1 if i % 10 == 0 else int(rng.integers(1, 9))
    C = 1 if i % 10 in (0, 1) else int(rng.integers(1, 9))
    return rng.integers(0, K, n), rng.integers(0, C, n), K, C


def test_scores_equal_scikit_learn_on_200_random_tables():
    from sklearn.metrics import adjusted_rand_score, normalized_mutual_info_score
    worst = 0.0
    for i in range(200):
        pred, truth, K, C = random_labels(i)
        table, skipped = ref.contingency(pred, truth, K, C)
        s = ref.scores(table)
        assert skipped == 0 and s.n == len(pred)
        d = max(abs(s.nmi - normalized_mutual_info_score(truth, pred)), abs(s.ari - adjusted_rand_score(truth, pred)))
        worst = max(worst, d)
        assert d <= 1e-12, (i, K, C, s.nmi, s.ari)
        assert s.purity == table.max(axis=1).sum() / len(pred)
    print("worst difference to scikit-learn: %.3g" % worst)


def test_scores_special_cases():
    assert np.isnan(ref.scores(np.zeros((3, 2), np.int64)).nmi)
    one = ref.scores(np.array([[5]]))
    assert one.nmi == 1.0 and one.ari == 1.0 and one.purity == 1.0
    table, skipped = ref.contingency([0, 1, -1, 2, 5], [0, 1, 1, 7, 0], 3, 2)
    assert skipped == 3 and table.tolist() == [[1, 0], [0, 1], [0, 0]]


@pytest.mark.parametrize("variant", ("rand_index", "nmi_geometric"))
def test_score_checker_is_decisive(variant):
    rng = np.random.default_rng(5)
    table, _ = ref.contingency(rng.integers(0, 4, 300), rng.integers(0, 6, 300), 4, 6)
    good, bad = ref.scores(table), ref.scores(table, variant)
    assert ref.check_scores(np.array([good.nmi, good.ari, good.purity, good.n]), table) is None
    assert ref.check_scores(np.array([bad.nmi, bad.ari, bad.purity, bad.n]), table) is not None


# ---- the checkers against the named wrong implementations -------------------------------------------------------------------------
def integer_case(metric, N=129, D=17, K=5, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.integers(-3, 4, (N, D)).astype(np.float32)
    X[X.any(axis=1) == 0, 0] = 1
    m = rng.integers(-3, 4, (K, D)).astype(np.float32)
    m[m.any(axis=1) == 0, 0] = 1
    m[K - 1] = m[0]                 # a planted duplicate: the tie goes to cluster 0
    return X, m


@pytest.mark.parametrize("metric", (ref.COSINE, ref.EUCLIDEAN))
def test_assign_checker_accepts_the_definition_and_names_wrong_labels(metric):
    X, m = integer_case(metric)
    X[7] = np.nan
    p = ref.prepare(X, metric)
    a = ref.assign(p, m)
    assert ref.check_assign(a.label, a.key, p, m) is None and a.label[7] == -1 and (a.label != m.shape[0] - 1).all()
    assert ref.check_assign(a.label, a.key, p, m, exact=True) is None
    high = ref.assign(p, m, variant="ties_high")
    assert (high.label == m.shape[0] - 1).any()
    # (the tolerant checker cannot tell equal keys apart; the exact one, which the integer cases run under, does)
    assert ref.check_assign(high.label, high.key, p, m, exact=True) is not None
    dead = ref.assign(p, m, variant="dead_assigned")
    assert "dead row 7" in ref.check_assign(dead.label, dead.key, p, m)


def test_assign_checker_names_a_missing_euclidean_offset():
    X, m = integer_case(ref.EUCLIDEAN)
    m[1] *= 3
    p = ref.prepare(X, ref.EUCLIDEAN)
    bad = ref.assign(p, m, variant="no_offset")
    assert ref.check_assign(bad.label, bad.key, p, m) is not None


def members_case(metric, K=3, D=5):
    """cluster sizes 2 CHUNK + 1, 0 and CHUNK + 1"""
    rng = np.random.default_rng(2)
    label = np.array([0] * (2 * ref.CHUNK + 1) + [2] * (ref.CHUNK + 1))
    rng.shuffle(label)
    X = rng.standard_normal((len(label), D)).astype(np.float32) + 2
    prev = rng.standard_normal((K, D)).astype(np.float32)
    return ref.prepare(X, metric), label, prev


@pytest.mark.parametrize("variant,metric", (("nonorm_centroid", ref.COSINE), ("empty_zeroed", ref.COSINE),
                                            ("empty_zeroed", ref.EUCLIDEAN), ("chunk_edge", ref.EUCLIDEAN),
                                            ("chunk_edge", ref.COSINE)))
def test_update_checker_is_decisive(variant, metric):
    p, label, prev = members_case(metric)
    good, bad = ref.update(p, label, prev), ref.update(p, label, prev, variant)
    assert ref.check_update(good.m, good.count, good.empty, p, label, prev) is None
    assert good.empty == 1 and (good.m[1] == prev[1]).all()
    assert ref.check_update(bad.m, bad.count, bad.empty, p, label, prev) is not None


def test_update_keeps_the_centroid_of_an_antipodal_cluster():
    X = np.array([[1, 2, 3], [-1, -2, -3], [0, 1, 0]], np.float32)
    p = ref.prepare(X, ref.COSINE)
    prev = np.array([[1, 0, 0], [0, 0, 1]], np.float32)
    u = ref.update(p, np.array([0, 0, 1]), prev)
    assert u.empty == 1 and (u.m[0] == prev[0]).all() and u.count.tolist() == [2, 1] and u.m[1].tolist() == [0, 1, 0]


def test_inertia_belongs_to_the_returned_centroids():
    X, _ = ref.blobs(300, 17, 5, 1)
    r = ref.run(X, 5, ref.EUCLIDEAN, 2, seed=1)             # (stops before convergence: the centroids still move)
    a = ref.assign(r.p, r.centroid)
    assert (a.label == r.label).all() and a.inertia == r.inertia
    p = r.p
    chosen, m0 = ref.seed_centroids(p, 5, 1, 0)
    stale = ref.assign(p, r.centroid, variant="stale_inertia", stale=m0)
    assert abs(stale.inertia - r.inertia) > 10 * ref.tol_inertia(a.cost) + 1e-6 * r.inertia


@pytest.mark.parametrize("metric", (ref.COSINE, ref.EUCLIDEAN))
def test_seed_checker_replays_and_names_the_closed_interval(metric):
    """the replay accepts the definition's picks, names a pick without weight and a pick next to the right one, and -- with
    the draw replaced so that t lands on a prefix sum -- the closed-interval rule"""
    X, _ = ref.blobs(65, 16, 2, 0)
    X[0] = np.inf
    p = ref.prepare(X, metric)
    for seed in range(4):
        chosen, m = ref.seed_centroids(p, 4, seed, 1)
        assert ref.check_seed(chosen, m, p, 4, seed, 1) is None
        assert (chosen > 0).all() and len(set(chosen.tolist())) == 4
        wrong = chosen.copy()
        wrong[2] = 0
        assert "no weight" in ref.check_seed(wrong, m, p, 4, seed, 1)
        shifted = chosen.copy()
        shifted[1] = chosen[1] + 1 if chosen[1] + 1 < p.N else chosen[1] - 1
        m2 = m.copy()
        m2[1] = p.z[shifted[1]]
        assert ref.check_seed(shifted, m2, p, 4, seed, 1) is not None
    # P_r >= t differs from P_r > t exactly when t equals a prefix sum: round 0's unit weights and a draw of 1/2 over 64 live
    # rows put t = 32 on P_31; the definition picks row 32 (+ 1 for the dead row 0), the wrong rule row 31
    half = lambda seed, restart, j: 0.5 if j == 0 else ref.draw(seed, restart, j)         # noqa: E731
    good, mg = ref.seed_centroids(p, 2, 0, 0, draw=half)
    bad, mb = ref.seed_centroids(p, 2, 0, 0, variant="pick_ge", draw=half)
    assert good[0] == 33 and bad[0] == 32
    assert ref.check_seed(good, mg, p, 2, 0, 0, draw=half) is None
    assert "pick 0" in ref.check_seed(bad, mb, p, 2, 0, 0, draw=half)


def test_seed_fallback_order():
    X = np.ones((5, 3), np.float32)
    X[0] = np.nan
    p = ref.prepare(X, ref.EUCLIDEAN)
    chosen, m = ref.seed_centroids(p, 7, 0, 0)
    assert chosen[0] in (1, 2, 3, 4)
    rest = [r for r in (1, 2, 3, 4) if r != chosen[0]]
    assert chosen[1:4].tolist() == rest and chosen[4:].tolist() == [1, 1, 1]       # the free rows, then the lowest live row
    none = ref.prepare(np.full((3, 2), np.nan, np.float32), ref.COSINE)
    chosen, m = ref.seed_centroids(none, 2, 0, 0)
    assert chosen.tolist() == [-1, -1] and not m.any()


# ---- decidable trajectories --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,seeds", ref.DECIDABLE)
@pytest.mark.parametrize("metric", (ref.COSINE, ref.EUCLIDEAN))
def test_blob_trajectories_are_decidable(shape, seeds, metric):
    """a condition, not a measurement: at every assignment every row's best key leads every other by LEAD (8) pair bounds, so
    whatever the MFMA rounds, the GPU's labels are these"""
    for seed in seeds:
        X, _ = ref.blobs(*shape, seed)
        r = ref.run(X, shape[2], metric, ref.DECIDABLE_ITERS, seed=seed)
        print(shape, seed, metric, "lead %.1f bounds, %d assignments" % (r.lead, r.iterations))
        assert r.lead >= ref.LEAD, (shape, seed, metric, r.lead)
        assert r.moved[r.iterations - 1] == 0 and r.dead == 0


@pytest.mark.parametrize("metric", (ref.COSINE, ref.EUCLIDEAN))
def test_restart_case_is_decidable_and_a_later_restart_wins(metric):
    shape, seed, K, iters, restarts = ref.RESTART_CASE
    X, _ = ref.blobs(*shape, seed)
    r = ref.run(X, K, metric, iters, restarts=restarts, seed=seed)
    assert r.lead >= ref.LEAD and r.restart > 0 and r.moved[r.iterations - 1] == 0
    # the winner's inertia is below every other restart's by more than both bounds: the GPU picks the same restart
    for rho in range(restarts):
        if rho != r.restart:
            assert r.inertias[rho] - r.inertia > 2 * (r.tols[rho] + r.tol_inertia), (rho, r.inertias, r.tols)


# ---- what needs no device ----------------------------------------------------------------------------------------------------------
def test_workspace_formula_and_plan_are_the_headers():
    for N, D, K, iters in ((0, 1, 1, 0), (1, 1, 1, 1), (63, 15, 2, 3), (65, 17, 129, 50), (129, 33, 257, 7), (2708, 256, 7, 50),
                           (1_000_000, 256, 1024, 20)):
        assert ref.workspace_bytes(N, D, K, iters) == ref.workspace_formula(N, D, K, iters), (N, D, K, iters)
        assert ref.workspace_bytes(N, D, K, iters) % 8 == 0
        assert ref.plan(N, D, K) == (-(-N // 64), 64, 128, 16, ref.CHUNK, ref.BLOCK)
    # nothing in it is N x K: at a million rows and 1024 clusters the explicit fp32 matrix alone would be 4 GB
    assert ref.workspace_bytes(1_000_000, 256, 1024, 20) < 4 * 1_000_000 * 256 + 4 * 1_000_000 * 1024 // 2


def test_refusals_need_no_device():
    from pathnet_amd import _lib
    lib = _lib.load()
    need, out = ctypes.c_int64(-7), (ctypes.c_int64 * 6)(*([-7] * 6))
    for N, D, K, iters in ((-1, 4, 2, 0), (2 ** 31, 4, 2, 0), (5, 0, 2, 0), (5, 8193, 2, 0), (5, 4, 0, 0), (5, 4, ref.MAX_K + 1, 0),
                           (5, 4, 2, -1), (5, 4, 2, 65537)):
        assert lib.pn_kmeans_workspace_bytes(N, D, K, iters, ctypes.byref(need)) == _lib.PN_ERR_ARG
        if 0 <= iters <= 65536:
            assert lib.pn_kmeans_plan(N, D, K, out) == _lib.PN_ERR_ARG
        assert need.value == -7 and list(out) == [-7] * 6
    assert lib.pn_kmeans_workspace_bytes(5, 4, 2, 0, None) == _lib.PN_ERR_ARG
    assert lib.pn_kmeans_plan(5, 4, 2, None) == _lib.PN_ERR_ARG
    assert _lib.KMEANS_MAX_K == ref.MAX_K and _lib.KMEANS_STREAM == ref.STREAM
    # every entry point refuses before it touches a device: host memory stands in for the device pointers
    N, D, K = 5, 4, 2
    bytes_ = ref.workspace_bytes(N, D, K, 3)
    buf = np.zeros(bytes_ // 8 + 2, np.int64)
    ws, x = buf.ctypes.data, np.zeros((N, D), np.float32).ctypes.data
    aout, rout = _lib.KmeansAssignOut(), _lib.KmeansOut()
    E = _lib.PN_ERR_ARG
    assert lib.pn_kmeans_prepare(None, x, D, N, D, K, 2, None, ws, bytes_, None, None) == E         # metric
    assert lib.pn_kmeans_prepare(None, x, D - 1, N, D, K, 0, None, ws, bytes_, None, None) == E     # stride
    assert lib.pn_kmeans_prepare(None, None, D, N, D, K, 0, None, ws, bytes_, None, None) == E      # NULL X
    assert lib.pn_kmeans_prepare(None, x, D, N, D, K, 0, None, None, bytes_, None, None) == E       # NULL workspace
    assert lib.pn_kmeans_prepare(None, x, D, N, D, K, 0, None, ws, 64, None, None) == E             # short
    assert lib.pn_kmeans_prepare(None, x, D, N, D, K, 0, None, ws + 4, bytes_, None, None) == E     # misaligned
    assert lib.pn_kmeans_set_centroids(None, None, D, N, D, K, ws, bytes_, None) == E
    assert lib.pn_kmeans_set_centroids(None, x, D - 1, N, D, K, ws, bytes_, None) == E
    assert lib.pn_kmeans_seed(None, N, D, K, 0, 0, -1, ws, bytes_, None, None, None) == E
    assert lib.pn_kmeans_seed(None, N, D, K, 0, 0, 0, ws, 64, None, None, None) == E
    assert lib.pn_kmeans_assign(None, N, D, K, 0, ws, bytes_, None, 16, ctypes.byref(aout), None, None) == E   # label width
    assert lib.pn_kmeans_assign(None, N, D, K, 0, ws, bytes_, None, 32, None, None, None) == E
    assert lib.pn_kmeans_assign(None, N, D, K + 2000, 0, ws, bytes_, None, 32, ctypes.byref(aout), None, None) == E
    assert lib.pn_kmeans_update(None, N, D, K, 0, ws, bytes_, None, 32, None, None, None, None, None) == E       # NULL labels
    assert lib.pn_kmeans_update(None, N, D, K, 5, ws, bytes_, x, 32, None, None, None, None, None) == E
    run = lambda **kw: lib.pn_kmeans_run(None, kw.get("x", x), D, N, D, K, 0, None, kw.get("init"), D, kw.get("iters", 3),  # noqa: E731
                                         kw.get("restarts", 1), 0, ws, kw.get("bytes", bytes_), 64,
                                         ctypes.byref(rout) if kw.get("out", True) else None, None)
    assert run(iters=0) == E and run(restarts=0) == E and run(init=x, restarts=2) == E and run(x=None) == E
    assert run(out=False) == E and run(bytes=bytes_ - 8) == E and run(iters=4) == E          # (iters = 4 needs 8 more bytes)
    t = np.zeros(4, np.int64).ctypes.data
    assert lib.pn_cluster_scores(None, t, 0, t, 2, 2, t, None, None, None) == E
    assert lib.pn_cluster_scores(None, t, 2, t, 4097, 2, t, None, None, None) == E
    assert lib.pn_cluster_scores(None, t, 2, t, 2, -1, t, None, None, None) == E
    assert lib.pn_cluster_scores(None, t, 2, t, 2, 2, None, None, None, None) == E
    assert lib.pn_cluster_scores(None, None, 2, t, 2, 2, t, None, None, None) == E
    assert not buf.any()
