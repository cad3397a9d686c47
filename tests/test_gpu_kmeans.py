"""pn_kmeans_* and pn_cluster_scores on the GPU, through the C ABI, against the NumPy restatement tests/cluster_ref.py.

As in test_gpu_knn.py every input, workspace and output sits between two guard bands of 0xFF bytes that must come back
untouched, outputs start as 0xFF themselves, and with a row stride above D the padding behind every input row is NaN.

Held to (bounds and their derivation: cluster_ref's docstring): assign bit for bit on inputs whose fma chains are exact, at
every tile edge, by the tolerant checker on random inputs, and against pn_knn_search(k = 1) bit for bit; update bit for
bit on exact inputs and inside the bound on random ones, given the test's labels; k-means++ pick for pick; the scores' table
exactly and the scores inside their bound; whole runs label for label on the trajectories test_cluster_ref_host.py shows to
be decidable; every refusal with the outputs untouched.
"""
import ctypes

import numpy as np
import pytest
import torch

import cluster_ref as ref
import test_gpu_ensemble as tge
from test_gpu_contrast import padded
from test_gpu_knn import gpu_knn, guarded_of, read

pytestmark = pytest.mark.gpu

Guarded, lib_ctx = tge.Guarded, tge.lib_ctx
LABEL = {32: np.int32, 64: np.int64}


class Session:
    """one workspace: prepare at construction, then the single steps"""

    def __init__(self, X, K, metric, valid=None, pad=3):
        self._lib, self.lib, self.ctx, self.stream = lib_ctx()
        self.N, self.D = X.shape
        self.K, self.metric = K, metric
        self.bytes = ref.workspace_bytes(self.N, self.D, K)
        self.ws = Guarded(self.bytes)
        self.held = [self.ws]
        xg = padded(np.asarray(X, np.float32), self.D + pad)
        vg = guarded_of(np.asarray(valid, np.uint8)) if valid is not None else None
        counts = Guarded(8)
        self.call(self.lib.pn_kmeans_prepare, xg.ptr(), self.D + pad, self.N, self.D, K, metric, vg.ptr() if vg else None,
                  self.ws.ptr(), self.bytes, counts.ptr(), self.stream, watch=[xg, counts] + ([vg] if vg else []))
        self.dead = int(read(counts, np.int64, (1,))[0])

    def call(self, fn, *args, watch=()):
        self._lib.check(fn(self.ctx, *args))
        torch.cuda.synchronize()
        for g in self.held + list(watch):
            assert g.intact()

    def set_centroids(self, m, pad=2):
        mg = padded(np.asarray(m, np.float32), self.D + pad)
        self.call(self.lib.pn_kmeans_set_centroids, mg.ptr(), self.D + pad, self.N, self.D, self.K, self.ws.ptr(), self.bytes,
                  self.stream, watch=[mg])

    def seed(self, seed, restart):
        cg, hg = Guarded(4 * self.K * self.D), Guarded(8 * self.K)
        self.call(self.lib.pn_kmeans_seed, self.N, self.D, self.K, self.metric, seed, restart, self.ws.ptr(), self.bytes, cg.ptr(),
                  hg.ptr(), self.stream, watch=[cg, hg])
        return read(hg, np.int64, (self.K,)), read(cg, np.float32, (self.K, self.D))

    def assign(self, prev=None, bits=64, done=None):
        """-> (Result, the output buffers, the done flag afterwards)"""
        N = self.N
        bufs = dict(label=Guarded(max(bits // 8 * N, 4)), key=Guarded(max(8 * N, 4)), moved=Guarded(8), inertia=Guarded(8),
                    iterations=Guarded(4, fill=0))
        out = self._lib.KmeansAssignOut(*(bufs[f].ptr() for f in self._lib.KmeansAssignOut.FIELDS))
        pg = guarded_of(np.asarray(prev, LABEL[bits])) if prev is not None else None
        dg = guarded_of(np.array([done], np.int32)) if done is not None else None
        self.call(self.lib.pn_kmeans_assign, N, self.D, self.K, self.metric, self.ws.ptr(), self.bytes, pg.ptr() if pg else None,
                  bits, ctypes.byref(out), dg.ptr() if dg else None, self.stream,
                  watch=list(bufs.values()) + [g for g in (pg, dg) if g])
        got = ref.Result(label=read(bufs["label"], LABEL[bits], (N,)).astype(np.int64), key=read(bufs["key"], np.float64, (N,)),
                         moved=int(read(bufs["moved"], np.int64, (1,))[0]), inertia=float(read(bufs["inertia"], np.float64, (1,))[0]),
                         iterations=int(read(bufs["iterations"], np.int32, (1,))[0]))
        return got, bufs, (int(read(dg, np.int32, (1,))[0]) if dg else None)

    def update(self, label, bits=64, done=None):
        lg = guarded_of(np.asarray(label, LABEL[bits]))
        cg, ng, eg = Guarded(4 * self.K * self.D), Guarded(8 * self.K), Guarded(8)
        dg = guarded_of(np.array([done], np.int32)) if done is not None else None
        self.call(self.lib.pn_kmeans_update, self.N, self.D, self.K, self.metric, self.ws.ptr(), self.bytes, lg.ptr(), bits,
                  cg.ptr(), ng.ptr(), eg.ptr(), dg.ptr() if dg else None, self.stream, watch=[lg, cg, ng, eg] + ([dg] if dg else []))
        return read(cg, np.float32, (self.K, self.D)), read(ng, np.int64, (self.K,)), int(read(eg, np.int64, (1,))[0]), (ng, eg)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- assign ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (1, 2, 127, 128, 129, 257))
@pytest.mark.parametrize("metric", (ref.COSINE, ref.EUCLIDEAN))
def test_assign_is_bit_equal_on_exact_inputs_at_every_tile_edge(metric, K):
    """N at the row tile's edges, D at the K chunk's, K at the column tile's; planted duplicate centroids go to the lowest"""
    for N in (1, 63, 64, 65, 129):
        for D in (1, 15, 16, 17, 33):
            X, m = ref.exact_case(N, D, K, metric, seed=N + D)
            p = ref.prepare(X, metric)
            s = Session(X, K, metric)
            s.set_centroids(m)
            prev = np.arange(N) % K
            got, _, _ = s.assign(prev=prev, bits=32 if D % 2 else 64)
            want = ref.assign(p, m, prev)
            assert ref.check_assign(got.label, got.key, p, m, exact=True) is None, (N, D)
            assert K < 2 or not (got.label == K - 1).any()
            assert K < 129 or not (got.label == 128).any()
            assert got.moved == want.moved and got.inertia == want.inertia and got.iterations == 1 and s.dead == p.dead == 0


@pytest.mark.parametrize("metric", (ref.COSINE, ref.EUCLIDEAN))
@pytest.mark.parametrize("N,D,K", ((129, 33, 5), (65, 17, 129), (200, 40, 257)))
def test_assign_random_inputs_dead_rows_moved_and_inertia(metric, N, D, K):
    rng = np.random.default_rng(N + K)
    X = (rng.standard_normal((N, D)) * 3).astype(np.float32)
    m = rng.standard_normal((K, D)).astype(np.float32)
    valid = np.ones(N, np.uint8)
    X[3, D // 2], X[N - 1, 0], X[10] = np.nan, np.inf, 0.0      # (a zero row is dead for cosine only)
    valid[20] = 0
    p = ref.prepare(X, metric, valid)
    assert p.dead == (4 if metric == ref.COSINE else 3)
    s = Session(X, K, metric, valid)
    s.set_centroids(m)
    prev = ref.assign(p, m).label.copy()
    prev[::7] = -5              # planted: every seventh row differs, and so do the dead rows' entries -- which do not count
    got, _, _ = s.assign(prev=prev)
    assert s.dead == p.dead
    assert ref.check_assign(got.label, got.key, p, m) is None
    assert (got.label[~p.live] == -1).all() and np.isneginf(got.key[~p.live]).all()
    assert got.moved == int((p.live & (got.label != prev)).sum())
    cost = ref.costs(p, got.key)
    assert (cost[~p.live] == 0).all()
    assert abs(got.inertia - ref.blocked_sum(cost)[0]) <= ref.tol_inertia(cost)
    # no previous labels: every live row moved
    first, _, _ = s.assign()
    assert first.moved == int(p.live.sum()) and same_bits(first.label, got.label) and same_bits(first.key, got.key)


def test_assign_gives_nothing_to_a_centroid_that_is_not_live():
    rng = np.random.default_rng(1)
    X = rng.standard_normal((70, 6)).astype(np.float32)
    m = rng.standard_normal((4, 6)).astype(np.float32)
    m[0, 3], m[2] = np.nan, 0.0           # not finite; all zeros: dead under cosine, the origin under euclidean
    X[:8] *= 0.01                         # (close to the origin)
    for metric in (ref.COSINE, ref.EUCLIDEAN):
        p = ref.prepare(X, metric)
        s = Session(X, 4, metric, pad=0)
        s.set_centroids(m, pad=0)
        got, _, _ = s.assign()
        assert ref.check_assign(got.label, got.key, p, m) is None
        assert (got.label != 0).all() and ((got.label == 2).any() == (metric == ref.EUCLIDEAN))
    # no centroid is live: every live row takes the lowest cluster at a key of -inf
    s = Session(X, 2, ref.COSINE)
    s.set_centroids(np.zeros((2, 6), np.float32))
    got, _, _ = s.assign()
    assert (got.label == 0).all() and np.isneginf(got.key).all() and got.inertia == np.inf


@pytest.mark.parametrize("N,D,K", ((129, 17, 3), (65, 33, 130), (64, 16, 128)))
def test_cosine_assign_equals_the_nearest_neighbour_search(N, D, K):
    """pn_knn_search(k = 1) over centroids of unit norm (its own normalisation leaves them as they are) is the oracle: the
    same index, and the same score bits"""
    rng = np.random.default_rng(K)
    X = rng.standard_normal((N, D)).astype(np.float32)
    X[5] = 0
    m = ref.unit_patterns(rng, K, D)
    m[K - 1] = m[0]
    s = Session(X, K, ref.COSINE)
    s.set_centroids(m)
    got, _, _ = s.assign()
    nn, _ = gpu_knn(X, m, 1, 0)
    assert (got.label == nn.index[:, 0]).all() and got.label[5] == -1
    assert same_bits(got.key.astype(np.float32), nn.score[:, 0])


def test_a_set_done_flag_leaves_every_output_untouched():
    X, m = ref.exact_case(130, 17, 5, ref.EUCLIDEAN)
    s = Session(X, 5, ref.EUCLIDEAN)
    s.set_centroids(m)
    got, bufs, done = s.assign(prev=np.zeros(130), done=1)
    assert done == 1 and all(bufs[k].untouched() for k in ("label", "key", "moved", "inertia"))
    assert got.iterations == 0
    # a clear flag is set when nothing moved, and only then
    a, _, done = s.assign(done=0)
    assert done == 0 and a.moved == 130
    b, _, done = s.assign(prev=a.label, done=0)
    assert done == 1 and b.moved == 0 and same_bits(a.label, b.label)
    # update obeys it: centroids (read back through an assign), counts and the empty count stay
    _, _, _, (ng, eg) = s.update(a.label, done=1)
    assert ng.untouched() and eg.untouched()
    c, _, _ = s.assign()
    assert same_bits(c.key, a.key)


# ---- update ----------------------------------------------------------------------------------------------------------------------
def sized_labels(K, chunk, rng):
    """labels with cluster sizes 0, 1, chunk - 1, chunk, chunk + 1 and 2 chunk + 1 where K allows, two dead rows and one label
    outside [0, K)"""
    sizes = {1: [2 * chunk + 1], 2: [chunk + 1, chunk]}.get(K, [0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk + 1])
    where = np.linspace(0, K - 1, len(sizes)).astype(int) if K > 2 else np.arange(len(sizes))
    label = np.concatenate([np.full(n, c) for n, c in zip(sizes, where)] + [np.array([0, 0, K + 3])])
    rng.shuffle(label)
    return label.astype(np.int64)


@pytest.mark.parametrize("D", (1, 63, 64, 65, 257))
@pytest.mark.parametrize("K", (1, 2, 129))
@pytest.mark.parametrize("metric", (ref.COSINE, ref.EUCLIDEAN))
def test_update_at_chunk_edges(metric, K, D):
    chunk = ref.plan(100, D, K)[4]
    assert chunk == ref.CHUNK
    rng = np.random.default_rng(K + D)
    label = sized_labels(K, chunk, rng)
    N = len(label)
    dead = np.flatnonzero(label == 0)[:2] if K > 2 else np.flatnonzero(label == 0)[:2]
    prev = rng.standard_normal((K, D)).astype(np.float32)
    for kind in ("exact", "random"):
        X = ref.exact_case(N, D, 1, metric, seed=D)[0] if kind == "exact" else (rng.standard_normal((N, D)) + 1).astype(np.float32)
        X[dead] = np.nan
        p = ref.prepare(X, metric)
        s = Session(X, K, metric)
        s.set_centroids(prev)
        m, count, empty, _ = s.update(label, bits=64 if kind == "exact" else 32)
        want = ref.update(p, label, prev)
        assert ref.check_update(m, count, empty, p, label, prev) is None, kind
        kept = want.count == 0
        assert same_bits(m[kept], prev[kept]) and empty >= kept.sum()
        if kind == "exact":
            assert same_bits(m, want.m)
        # the order depends on the assignment alone: rows regrouped so that every cluster's members keep their order
        order = np.argsort(label, kind="stable")
        s2 = Session(X[order], K, metric, pad=0)
        s2.set_centroids(prev, pad=0)
        m2, count2, empty2, _ = s2.update(label[order])
        assert same_bits(m, m2) and same_bits(count, count2) and empty == empty2


def test_update_keeps_empty_and_antipodal_clusters_and_counts_them():
    X = np.array([[1, 2, 3], [-1, -2, -3], [0, 1, 0], [2, 4, 6], [-2, -4, -6]], np.float32)
    prev = np.array([[1, 0, 0], [0, 0, 1], [0.5, 0.5, 0], [0, 1, 0]], np.float32)
    label = np.array([0, 0, 1, 3, 3])
    s = Session(X, 4, ref.COSINE)
    s.set_centroids(prev)
    m, count, empty, _ = s.update(label)
    assert count.tolist() == [2, 1, 0, 2] and empty == 3
    assert same_bits(m[[0, 2, 3]], prev[[0, 2, 3]]) and m[1].tolist() == [0, 1, 0]
    e = Session(X, 4, ref.EUCLIDEAN)
    e.set_centroids(prev)
    m, count, empty, _ = e.update(label)
    assert empty == 1 and same_bits(m[2], prev[2]) and not m[0].any() and not m[3].any() and m[1].tolist() == [0, 1, 0]


# ---- k-means++ ---------------------------------------------------------------------------------------------------------------------
def test_seed_on_integer_rows_is_the_restatements():
    rng = np.random.default_rng(0)
    X = rng.integers(-5, 6, (300, 9)).astype(np.float32)
    X[17] = np.nan
    p = ref.prepare(X, ref.EUCLIDEAN)
    s = Session(X, 6, ref.EUCLIDEAN)
    seen = set()
    for seed in range(4):
        for restart in range(2):
            chosen, m = s.seed(seed, restart)
            want, wm = ref.seed_centroids(p, 6, seed, restart)
            assert chosen.tolist() == want.tolist() and same_bits(m, wm), (seed, restart)
            seen.add(tuple(chosen.tolist()))
    assert len(seen) == 8 and 17 not in {c for t in seen for c in t}


@pytest.mark.parametrize("metric", (ref.COSINE, ref.EUCLIDEAN))
@pytest.mark.parametrize("N,D,K", ((700, 40, 9), (257, 65, 3), (64, 1, 2)))
def test_seed_on_random_rows_replays(metric, N, D, K):
    rng = np.random.default_rng(N)
    X = rng.standard_normal((N, D)).astype(np.float32)
    valid = (np.arange(N) % 11 != 0).astype(np.uint8)
    p = ref.prepare(X, metric, valid)
    s = Session(X, K, metric, valid)
    chosen, m = s.seed(12345678901234, 3)
    assert ref.check_seed(chosen, m, p, K, 12345678901234, 3) is None
    assert p.live[chosen].all()


def test_seed_fallbacks():
    # all rows identical: after the first pick every distance is 0; the lowest live rows not yet chosen, then the lowest
    X = np.ones((6, 4), np.float32)         # (four entries of 1/2: <z, z> is exactly 1)
    X[0] = np.nan
    for metric in (ref.COSINE, ref.EUCLIDEAN):
        p = ref.prepare(X, metric)
        s = Session(X, 8, metric)
        chosen, m = s.seed(1, 0)
        want, wm = ref.seed_centroids(p, 8, 1, 0)
        assert chosen.tolist() == want.tolist() and same_bits(m, wm)
        first = chosen[0]
        assert chosen[1:5].tolist() == [r for r in range(1, 6) if r != first] and chosen[5:].tolist() == [1, 1, 1]
    # K greater than the live rows of distinct data: picks repeat once the weights are all 0
    Y = np.arange(12, dtype=np.float32).reshape(4, 3) + 1
    s = Session(Y, 6, ref.EUCLIDEAN)
    chosen, m = s.seed(2, 0)
    assert sorted(chosen[:4].tolist()) == [0, 1, 2, 3] and chosen[4:].tolist() == [0, 0]
    assert ref.check_seed(chosen, m, ref.prepare(Y, ref.EUCLIDEAN), 6, 2, 0) is None
    # no live row
    s = Session(np.full((3, 4), np.inf, np.float32), 2, ref.COSINE)
    chosen, m = s.seed(0, 0)
    assert chosen.tolist() == [-1, -1] and not m.any() and s.dead == 3


# ---- scores ----------------------------------------------------------------------------------------------------------------------
def gpu_scores(pred, truth, K, C, table=None):
    _lib, lib, ctx, stream = lib_ctx()
    S = len(pred)
    pg, tg = guarded_of(np.asarray(pred, np.int64)), guarded_of(np.asarray(truth, np.int64))
    tab = table if table is not None else Guarded(8 * K * C, fill=0)
    sk, sc = Guarded(8, fill=0), Guarded(32)
    _lib.check(lib.pn_cluster_scores(ctx, pg.ptr(), K, tg.ptr(), C, S, tab.ptr(), sk.ptr(), sc.ptr(), stream))
    torch.cuda.synchronize()
    assert all(g.intact() for g in (pg, tg, tab, sk, sc))
    return read(tab, np.int64, (K, C)), int(read(sk, np.int64, (1,))[0]), read(sc, np.float64, (4,)), tab


@pytest.mark.parametrize("K,C", ((1, 1), (7, 7), (130, 7), (7, 130), (1, 130)))
@pytest.mark.parametrize("S", (0, 1, 257))
def test_scores(S, K, C):
    rng = np.random.default_rng(S + K + C)
    pred, truth = rng.integers(-1, K + 1, S), rng.integers(-1, C + 1, S)
    table, skipped, scores, _ = gpu_scores(pred, truth, K, C)
    want = np.zeros((K, C), np.int64)
    ok = (pred >= 0) & (pred < K) & (truth >= 0) & (truth < C)
    np.add.at(want, (pred[ok], truth[ok]), 1)
    assert (table == want).all() and skipped == int((~ok).sum())
    assert ref.check_scores(scores, want) is None, scores


def test_scores_accumulate_across_calls_and_known_values():
    rng = np.random.default_rng(9)
    pred, truth = rng.integers(0, 7, 514), rng.integers(0, 5, 514)
    _, _, _, tab = gpu_scores(pred[:257], truth[:257], 7, 5)
    table, _, scores, _ = gpu_scores(pred[257:], truth[257:], 7, 5, table=tab)
    want, _ = ref.contingency(pred, truth, 7, 5)
    assert (table == want).all() and ref.check_scores(scores, want) is None and scores[3] == 514
    # a relabelled copy is a perfect grouping; one cluster against two classes knows nothing
    _, _, perfect, _ = gpu_scores((truth + 2) % 7, truth, 7, 5)
    assert abs(perfect[0] - 1) < 1e-14 and perfect[1] == 1.0 and perfect[2] == 1.0
    _, _, nothing, _ = gpu_scores(np.zeros(4), np.array([0, 0, 1, 1]), 1, 2)
    assert nothing[0] == 0.0 and nothing[1] == 0.0 and nothing[2] == 0.5


# ---- whole runs --------------------------------------------------------------------------------------------------------------------
def run_bytes(c):
    return b"".join(t.cpu().numpy().tobytes() for t in c)


def check_run(got, want, metric):
    assert got.label.cpu().numpy().tolist() == want.label.tolist()
    assert got.count.cpu().numpy().tolist() == want.count.tolist()
    assert int(got.iterations) == want.iterations and got.moved.cpu().numpy().tolist() == want.moved.tolist()
    assert int(got.counts) == want.dead
    # the centroids: the last update's inside its bound, or the starting rows themselves when there was none
    m = got.centroid.cpu().numpy()
    if want.update is None:
        assert same_bits(m, want.centroid)
    else:
        assert (np.abs(m.astype(np.float64) - want.centroid) <= ref.tol_centroid(want.p, want.update)).all()
    inertia = float(got.inertia)
    assert abs(inertia - want.inertia) <= want.tol_inertia, (inertia, want.inertia, want.tol_inertia)


@pytest.mark.parametrize("shape,seeds", ref.DECIDABLE)
@pytest.mark.parametrize("metric", ("cosine", "euclidean"))
def test_whole_runs_equal_the_restatement(metric, shape, seeds):
    import pathnet_amd
    for seed in seeds:
        X, _ = ref.blobs(*shape, seed)
        want = ref.run(X, shape[2], pathnet_amd.cluster.METRICS[metric], ref.DECIDABLE_ITERS, seed=seed)
        x = torch.from_numpy(X).cuda()
        got = pathnet_amd.kmeans(x, shape[2], metric=metric, iters=ref.DECIDABLE_ITERS, seed=seed)
        check_run(got, want, metric)
        again = pathnet_amd.kmeans(x, shape[2], metric=metric, iters=ref.DECIDABLE_ITERS, seed=seed)
        assert run_bytes(got) == run_bytes(again)
    s = got.summary()
    assert s["converged"] and s["iterations"] == want.iterations and s["dead_rows"] == 0 and s["moved"][-1] == 0


@pytest.mark.parametrize("metric", ("cosine", "euclidean"))
def test_restarts_return_the_restart_the_restatement_picks(metric):
    import pathnet_amd
    shape, seed, K, iters, restarts = ref.RESTART_CASE
    X, _ = ref.blobs(*shape, seed)
    want = ref.run(X, K, pathnet_amd.cluster.METRICS[metric], iters, restarts=restarts, seed=seed)
    assert want.restart > 0
    x = torch.from_numpy(np.concatenate((X, np.full((len(X), 3), np.nan, np.float32)), axis=1)).cuda()[:, :shape[1]]
    got = pathnet_amd.kmeans(x, K, metric=metric, iters=iters, restarts=restarts, seed=seed)      # (a row-strided view)
    check_run(got, want, metric)
    assert run_bytes(got) == run_bytes(pathnet_amd.kmeans(x, K, metric=metric, iters=iters, restarts=restarts, seed=seed))
    one = pathnet_amd.kmeans(x, K, metric=metric, iters=iters, restarts=1, seed=seed)
    assert float(got.inertia) < float(one.inertia)


@pytest.mark.parametrize("metric", ("cosine", "euclidean"))
def test_a_caller_init_tensor_and_invalid_rows(metric):
    import pathnet_amd
    code = pathnet_amd.cluster.METRICS[metric]
    X, _ = ref.blobs(300, 17, 5, 2)
    valid = np.arange(300) % 13 != 0
    p = ref.prepare(X, code, valid)
    _, init = ref.seed_centroids(p, 5, 99, 0)
    want = ref.run(X, 5, code, 10, init=init, valid=valid)
    assert want.lead >= ref.LEAD
    x = torch.from_numpy(X).cuda()
    got = pathnet_amd.kmeans(x.double(), 5, metric=metric, iters=10, init=torch.from_numpy(init).cuda(), valid=torch.from_numpy(valid))
    check_run(got, want, metric)
    assert (got.label.cpu().numpy()[~valid] == -1).all() and int(got.counts) == int((~valid).sum())
    with pytest.raises(ValueError, match="restarts"):
        pathnet_amd.kmeans(x, 5, init=torch.from_numpy(init).cuda(), restarts=2)
    for kw, word in ((dict(clusters=0), "clusters=0"), (dict(clusters=1025), "clusters=1025"), (dict(clusters=2, metric="l1"), "metric"),
                     (dict(clusters=2, iters=0), "iters"), (dict(clusters=2, restarts=0), "restarts"),
                     (dict(clusters=2, init="random"), "init"), (dict(clusters=2, valid=torch.ones(5)), "valid")):
        with pytest.raises(ValueError, match=word):
            pathnet_amd.kmeans(x, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pathnet_amd.kmeans(x.cpu(), 2)
    empty = pathnet_amd.kmeans(x[:0], 3)
    assert empty.summary() == dict(rows=0, clusters=3, inertia=0.0, iterations=1, converged=True, dead_rows=0, empty_clusters=3,
                                   largest=0, moved=[0]) and not empty.centroid.any()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    _lib, lib, ctx, stream = lib_ctx()
    N, D, K = 70, 9, 3
    X = np.ones((N, D), np.float32)
    bytes_ = ref.workspace_bytes(N, D, K, 4)
    ws, xg, cg = Guarded(bytes_), padded(X, D), Guarded(8)
    outs = dict(label=Guarded(8 * N), centroid=Guarded(4 * K * D), count=Guarded(8 * K), inertia=Guarded(8), iterations=Guarded(4),
                moved=Guarded(32), counts=Guarded(8), restart=Guarded(4))
    rout = _lib.KmeansOut(*(outs[f].ptr() for f in _lib.KmeansOut.FIELDS))
    aouts = dict(label=Guarded(8 * N), key=Guarded(8 * N), moved=Guarded(8), inertia=Guarded(8), iterations=Guarded(4))
    aout = _lib.KmeansAssignOut(*(aouts[f].ptr() for f in _lib.KmeansAssignOut.FIELDS))
    E = _lib.PN_ERR_ARG
    w, b = ws.ptr(), bytes_
    off = ctypes.c_void_p(w.value + 4)
    run = lambda n=N, d=D, k=K, metric=0, x=xg.ptr(), ld=D, init=None, iters=4, restarts=1, wsp=w, wb=b, bits=64, out=ctypes.byref(rout): \
        lib.pn_kmeans_run(ctx, x, ld, n, d, k, metric, None, init, d, iters, restarts, 0, wsp, wb, bits, out, stream)   # noqa: E731
    for kw in (dict(n=-1), dict(n=2 ** 31), dict(d=0), dict(d=8193), dict(k=0), dict(k=1025), dict(metric=2), dict(ld=D - 1),
               dict(x=None), dict(iters=0), dict(restarts=0), dict(init=xg.ptr(), restarts=2), dict(wsp=None), dict(wb=b - 8),
               dict(wsp=off), dict(bits=16), dict(out=None), dict(iters=65537)):
        assert run(**kw) == E, kw
    assert lib.pn_kmeans_prepare(ctx, xg.ptr(), D - 1, N, D, K, 0, None, w, b, cg.ptr(), stream) == E
    assert lib.pn_kmeans_prepare(ctx, xg.ptr(), D, N, D, K, 7, None, w, b, cg.ptr(), stream) == E
    assert lib.pn_kmeans_set_centroids(ctx, None, D, N, D, K, w, b, stream) == E
    assert lib.pn_kmeans_seed(ctx, N, D, K, 0, 0, -1, w, b, outs["centroid"].ptr(), outs["count"].ptr(), stream) == E
    assert lib.pn_kmeans_seed(ctx, N, D, K, 0, 0, 0, w, 64, outs["centroid"].ptr(), outs["count"].ptr(), stream) == E
    assert lib.pn_kmeans_assign(ctx, N, D, K, 0, w, b, None, 8, ctypes.byref(aout), None, stream) == E
    assert lib.pn_kmeans_assign(ctx, N, D, K, 0, off, b, None, 64, ctypes.byref(aout), None, stream) == E
    assert lib.pn_kmeans_update(ctx, N, D, K, 0, w, b, None, 64, outs["centroid"].ptr(), outs["count"].ptr(), cg.ptr(), None, stream) == E
    assert lib.pn_kmeans_update(ctx, N, D, K, 0, w, 128, aouts["label"].ptr(), 64, outs["centroid"].ptr(), outs["count"].ptr(),
                                cg.ptr(), None, stream) == E
    t = Guarded(8 * 6)
    assert lib.pn_cluster_scores(ctx, t.ptr(), 0, t.ptr(), 2, 3, t.ptr(), cg.ptr(), outs["moved"].ptr(), stream) == E
    assert lib.pn_cluster_scores(ctx, t.ptr(), 3, t.ptr(), 4097, 3, t.ptr(), cg.ptr(), outs["moved"].ptr(), stream) == E
    assert lib.pn_cluster_scores(ctx, None, 3, t.ptr(), 2, 3, t.ptr(), cg.ptr(), outs["moved"].ptr(), stream) == E
    assert lib.pn_cluster_scores(ctx, t.ptr(), 3, t.ptr(), 2, 3, None, cg.ptr(), outs["moved"].ptr(), stream) == E
    torch.cuda.synchronize()
    assert all(g.untouched() for g in list(outs.values()) + list(aouts.values()) + [ws, cg, t]) and xg.intact()
