"""model.cluster_probe() on a small planted-partition graph built here as test_gpu_knn_probe.py builds its own (240 nodes in 3
blocks; W = 8, L = 3, H = 32, F = 16 -- L = 4 for PAGG, whose distance bank has four layers whatever it is given): the probe against embed(), kmeans() and cluster_scores() composed by hand, bit for
bit; labels per node of X against labels per node of the list; the host-side accuracy of summary() against
linear_sum_assignment on the table read back."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, F, W, H, C = 240, 16, 8, 32, 3
SEED = 5


def walk_len(name):
    return 4 if name == "PAGG" else 3


@functools.lru_cache(None)
def graph(L):
    """-> (sampler, X on the GPU, block of every node): edges inside a block with probability 0.08, across with 0.004; the
    features carry the block's signal in 2 columns of their own plus unit noise"""
    import pathnet_amd
    rng = np.random.default_rng(6)
    block = (np.arange(N) * C // N).astype(np.int64)
    prob = np.where(block[:, None] == block[None, :], 0.08, 0.004)
    adj = np.triu(rng.random((N, N)) < prob, 1)
    adj = adj | adj.T | np.eye(N, dtype=bool)
    src, dst = np.nonzero(adj)
    p = 1.0 / adj.sum(axis=1)[src]
    smp = pathnet_amd.MerwSampler(N, src.astype(np.int32), dst.astype(np.int32), p, L)
    signal = 4.0 * (np.arange(F)[None, :] // 2 == block[:, None])
    X = torch.from_numpy((rng.standard_normal((N, F)) + signal).astype(np.float32))
    return smp, X.cuda(), block


def model_of(name, seed=3):
    import pathnet_amd
    torch.manual_seed(seed)
    return getattr(pathnet_amd, name)(F, H, C, walk_len(name)).cuda()


@pytest.mark.parametrize("name", ("PathNet_homo", "PAGG", "PathNet"))
def test_cluster_probe_equals_the_composition(name):
    import pathnet_amd
    L = walk_len(name)
    smp, X, block = graph(L)
    m = model_of(name)
    nodes = torch.arange(N, dtype=torch.int32, device="cuda")[3:231:2].contiguous()
    y = torch.from_numpy(block).cuda()
    y_some = y.clone()
    y_some[::10] = -1                       # unlabelled nodes: skipped by the scores, clustered all the same
    kw = dict(samples=2, seed=SEED, first_epoch=1, batch_nodes=50)
    found, scores = m.cluster_probe(X, smp, W, L, nodes, y_some, clusters=4, metric="euclidean", iters=15, restarts=2, **kw)
    z = m.embed(X, smp, W, L, nodes, **kw)
    want = pathnet_amd.kmeans(z, 4, metric="euclidean", iters=15, restarts=2, seed=SEED)
    for a, b in zip(found, want):
        assert torch.equal(a, b)
    yl = y_some[nodes.long()]
    want_scores = pathnet_amd.cluster_scores(want.label, yl, 4, C)
    for a, b in zip(scores, want_scores):
        assert torch.equal(a, b) or (torch.isnan(a).all() and torch.isnan(b).all())
    assert int(scores.skipped) == int((yl < 0).sum()) and float(scores.n) == float((yl >= 0).sum())
    assert scores.table.shape == (4, C) and int(scores.table.sum()) == int((yl >= 0).sum())
    # labels per node of the list give the same; the defaults (cosine, clusters = out_size, four restarts); no labels at all
    per_list, s2 = m.cluster_probe(X, smp, W, L, nodes, yl, clusters=4, metric="euclidean", iters=15, restarts=2, **kw)
    assert torch.equal(per_list.label, found.label) and torch.equal(s2.table, scores.table)
    plain, none = m.cluster_probe(X, smp, W, L, nodes, seed=SEED)
    assert none is None and plain.centroid.shape == (C, z.shape[1]) and plain.moved.shape == (50,)
    w2 = pathnet_amd.kmeans(m.embed(X, smp, W, L, nodes, seed=SEED), C, restarts=4, seed=SEED)
    assert torch.equal(plain.label, w2.label) and torch.equal(plain.inertia, w2.inertia)
    with pytest.raises(ValueError, match="labels"):
        m.cluster_probe(X, smp, W, L, nodes, y[:17])


def test_all_nodes_with_a_list_of_n_entries_reads_labels_per_node_of_x():
    """N labels are per node of X and picked by node id, also where the list itself has N entries (knn_probe()'s rule)"""
    L = walk_len("PathNet_homo")
    smp, X, block = graph(L)
    m = model_of("PathNet_homo")
    y = torch.from_numpy(block).cuda()
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(0)).to(device="cuda", dtype=torch.int32)
    found, scores = m.cluster_probe(X, smp, W, L, perm, y, seed=SEED, iters=20)
    import pathnet_amd
    want = pathnet_amd.cluster_scores(found.label, y[perm.long()], C, C)
    assert torch.equal(scores.table, want.table)


def test_summary_accuracy_is_the_best_one_to_one_match_of_the_table():
    from scipy.optimize import linear_sum_assignment
    import pathnet_amd
    L = walk_len("PAGG")
    smp, X, block = graph(L)
    m = model_of("PAGG")
    found, scores = m.cluster_probe(X, smp, W, L, None, block, clusters=5, seed=SEED, iters=20)
    s = scores.summary()
    table = scores.table.cpu().numpy()
    rows, cols = linear_sum_assignment(-table)
    assert s["n"] == N == int(table.sum()) and s["skipped"] == 0 and s["accuracy_computed_on"] == "host"
    assert s["accuracy"] == table[rows, cols].sum() / N and s["match"] == {int(r): int(c) for r, c in zip(rows, cols)}
    assert s["nmi"] == float(scores.nmi) and s["ari"] == float(scores.ari) and s["purity"] == float(scores.purity)
    assert s["accuracy"] <= s["purity"] <= 1.0
    # a hand-made table: clusters 0 and 2 both hold class 1; one of them must take another class
    pred = torch.tensor([0, 0, 0, 2, 2, 1, 1, 2], device="cuda")
    truth = torch.tensor([1, 1, 1, 1, 1, 0, 0, 2], device="cuda")
    hand = pathnet_amd.cluster_scores(pred, truth, 3, 3).summary()
    assert hand["purity"] == 7 / 8 and hand["accuracy"] == 6 / 8 and hand["match"] == {0: 1, 1: 0, 2: 2}
    kept = pathnet_amd.cluster_scores(pred, truth, 3, 3, table=scores.table.new_zeros((3, 3)) + 1)
    assert int(kept.table.sum()) == 17
    with pytest.raises(ValueError, match="table"):
        pathnet_amd.cluster_scores(pred, truth, 3, 3, table=torch.zeros((3, 2), dtype=torch.int64, device="cuda"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pathnet_amd.cluster_scores(pred.cpu(), truth.cpu(), 3, 3)
