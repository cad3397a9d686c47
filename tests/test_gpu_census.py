"""The path-pattern census on the GPU (pn_census.hip through pathnet_amd.synth.PatternCensus) against the goldens recorded
from the reference programs and against the NumPy / scipy.sparse recurrence of census_ref.py.  Every comparison is exact."""
import numpy as np
import pytest
import torch

import census_ref
from conftest import golden
from pathnet_amd import PatternCensus, synth

pytestmark = pytest.mark.gpu

GOLDENS = ("census_small.npz", "census_cora.npz", "census_citeseer.npz")


def random_rows(n, m, seed, loops=0, repeats=0):
    rng = np.random.default_rng(seed)
    u, v = rng.integers(0, n, m), rng.integers(0, n, m)
    if loops:
        u[:loops] = v[:loops]
    if repeats:
        u, v = np.concatenate([u, u[-repeats:]]), np.concatenate([v, v[-repeats:]])
    return u.astype(np.int32), v.astype(np.int32)


def lowest_argmax(counts):
    """torch, on the device: the lowest index among the largest counts of every row."""
    top = counts.max(dim=1, keepdim=True).values
    idx = torch.arange(counts.shape[1], device=counts.device).expand_as(counts)
    return torch.where(counts == top, idx, torch.full_like(idx, counts.shape[1])).min(dim=1).values


@pytest.mark.parametrize("name", GOLDENS)
def test_labels_equal_the_reference_programs(name):
    g = golden(name)
    cen = PatternCensus(int(g["n"]), g["u"], g["v"])
    lab = cen.labels(walk_len=3)
    assert lab.dtype == torch.int64 and lab.shape == (int(g["n"]),) and lab.is_cuda
    assert (lab.cpu().numpy() == g["labels"]).all()
    assert cen.fits_int32(3)
    own, _ = census_ref.entries(g["u"], g["v"])
    assert cen.max_list == int(np.bincount(own, minlength=int(g["n"])).max())
    assert cen.entries == 2 * len(g["u"])


def test_lists_are_the_undirected_multiset():
    g = golden("census_small.npz")
    n = int(g["n"])
    cen = PatternCensus(n, torch.from_numpy(g["u"]).cuda(), torch.from_numpy(g["v"]).cuda())     # rows already on the device
    off, adj = cen.d_off.cpu().numpy(), cen.d_adj.cpu().numpy()
    own, ent = census_ref.entries(g["u"], g["v"])
    assert off[0] == 0 and off[-1] == len(own) and (np.diff(off) == np.bincount(own, minlength=n)).all()
    for node in range(n):
        assert sorted(adj[off[node]:off[node + 1]].tolist()) == sorted(ent[own == node].tolist()), node


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6])
def test_counts_two_symbols(k):
    n = 4001                                             # odd: the last workgroup is not full
    u, v = random_rows(n, 3 * n, 11, loops=30, repeats=200)
    cen = PatternCensus(n, u, v)
    C = cen.counts(walk_len=k)
    assert C.dtype == torch.int64 and C.shape == (n, 2 ** k)
    assert (C.cpu().numpy() == census_ref.counts_sparse(n, u, v, k)).all()
    if k <= 3:
        assert (C.cpu().numpy() == census_ref.counts_numpy(n, u, v, k)).all()


def test_counts_three_symbols_random():
    n = 3000
    u, v = random_rows(n, 4 * n, 5, loops=10, repeats=50)
    sym = np.random.default_rng(1).integers(0, 3, n)
    cen = PatternCensus(n, u, v)
    want = census_ref.counts_sparse(n, u, v, 4, sym, 3)
    for s in (torch.from_numpy(sym), torch.from_numpy(sym.astype(np.uint8)).cuda(), sym.astype(np.int32)):
        assert (cen.counts(walk_len=4, symbols=s, num_symbols=3).cpu().numpy() == want).all()
    assert (cen.labels(walk_len=4, symbols=sym, num_symbols=3).cpu().numpy() == census_ref.labels_of(want)).all()


@pytest.mark.parametrize("B,k", [(2, 7), (2, 10), (3, 6), (16, 2), (4, 5)])
def test_counts_rows_of_512_bytes_and_more(B, k):
    """B^(k-1) >= 64: the lanes cover r instead of (entry, r)."""
    n = 2501
    u, v = random_rows(n, 2 * n, 3, loops=5, repeats=20)
    sym = np.random.default_rng(B * 100 + k).integers(0, B, n)
    cen = PatternCensus(n, u, v)
    want = census_ref.counts_sparse(n, u, v, k, sym, B)
    got = cen.counts(walk_len=k, symbols=sym, num_symbols=B)
    assert (got.cpu().numpy() == want).all()
    assert (cen.labels(walk_len=k, symbols=sym, num_symbols=B).cpu().numpy() == census_ref.labels_of(want)).all()


@pytest.mark.parametrize("name", GOLDENS)
def test_labels_are_the_lowest_argmax_of_counts(name):
    g = golden(name)
    cen = PatternCensus(int(g["n"]), g["u"], g["v"])
    for k in (1, 2, 3, 4):
        C = cen.counts(walk_len=k)
        assert int(((C == C.max(dim=1, keepdim=True).values).sum(dim=1) > 1).sum()) > 0        # ties exist
        assert torch.equal(cen.labels(walk_len=k), lowest_argmax(C))


def test_duplicated_rows_count_twice():
    n = 200
    u, v = random_rows(n, 500, 2)
    keep = np.unique(np.stack([np.minimum(u, v), np.maximum(u, v)]), axis=1)
    u1, v1 = keep[0].astype(np.int32), keep[1].astype(np.int32)                  # a simple graph
    u2, v2 = np.append(u1, u1[7]), np.append(v1, v1[7])                          # ... and one row of it twice
    c1, c2 = PatternCensus(n, u1, v1).counts(3).cpu().numpy(), PatternCensus(n, u2, v2).counts(3).cpu().numpy()
    assert (c1 == census_ref.counts_numpy(n, u1, v1, 3)).all()
    assert (c2 == census_ref.counts_numpy(n, u2, v2, 3)).all()
    assert (c1 != c2).any() and c2.sum() > c1.sum()
    # the row the other way round is the same duplicate
    c3 = PatternCensus(n, np.append(u1, v1[7]), np.append(v1, u1[7])).counts(3).cpu().numpy()
    assert (c3 == c2).all()


def test_star_with_100000_leaves_needs_int64():
    leaves, n = 100_000, 130_001
    ru, rv = random_rows(n, 150_000, 8, loops=100)
    u = np.concatenate([np.zeros(leaves, np.int32), ru])
    v = np.concatenate([np.arange(1, leaves + 1, dtype=np.int32), rv])
    cen = PatternCensus(n, u, v)
    assert cen.max_list >= leaves and not cen.fits_int32(3)
    want = census_ref.counts_sparse(n, u, v, 3)
    assert want.max() > 2 ** 31
    got = cen.counts(walk_len=3)
    assert (got.cpu().numpy() == want).all()
    assert (cen.labels(walk_len=3).cpu().numpy() == census_ref.labels_of(want)).all()


def test_one_million_nodes_of_degree_16():
    n = 1_000_000
    u, v = random_rows(n, 16 * n, 0)
    cen = PatternCensus(n, u, v)
    want = census_ref.counts_sparse(n, u, v, 3)
    lab = cen.labels(walk_len=3)
    assert (lab.cpu().numpy() == census_ref.labels_of(want)).all()
    assert (cen.counts(walk_len=3).cpu().numpy() == want).all()


def test_side_stream_without_host_synchronisation():
    n = 200_001
    u, v = random_rows(n, 8 * n, 4, loops=50, repeats=500)
    cen = PatternCensus(n, u, v)
    want = census_ref.counts_sparse(n, u, v, 4)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                       # four enqueues back to back, consumers included
        C = cen.counts(walk_len=4)
        lab = cen.labels(walk_len=4)
        C2 = cen.counts(walk_len=2)
        same = (lowest_argmax(C) == lab).all()
    side.synchronize()
    assert bool(same)
    assert (C.cpu().numpy() == want).all()
    assert (lab.cpu().numpy() == census_ref.labels_of(want)).all()
    assert (C2.cpu().numpy() == census_ref.counts_sparse(n, u, v, 2)).all()


def test_bad_rows_and_symbols_are_value_errors():
    u = np.array([0, 1, 2, 3], np.int32)
    for bad in (5, -1):
        v = np.array([1, 2, bad, 0], np.int32)
        with pytest.raises(ValueError, match="row 2"):
            PatternCensus(5, u, v)
        with pytest.raises(ValueError, match="row 2"):
            PatternCensus(5, v, u)
    cen = PatternCensus(5, u, np.array([1, 2, 3, 0], np.int32))
    with pytest.raises(ValueError, match="symbols"):
        cen.counts(3, symbols=np.array([0, 1, 2, 0, 1]), num_symbols=2)
    with pytest.raises(ValueError, match="symbols"):
        cen.counts(3, symbols=np.array([0, 1, -1, 0, 1]), num_symbols=2)
    with pytest.raises(ValueError, match="symbols"):
        cen.counts(3, symbols=np.array([0, 1, 0, 1]), num_symbols=2)
    with pytest.raises(TypeError):
        cen.counts(3, symbols=np.array([0.0, 1, 0, 1, 1]), num_symbols=2)
    for k, B in ((0, 2), (3, 1), (3, 17), (11, 2)):
        with pytest.raises(ValueError):
            cen.labels(walk_len=k, num_symbols=B)
    # an empty graph and a graph without rows
    assert PatternCensus(0, u[:0], u[:0]).labels(3).shape == (0,)
    lone = PatternCensus(3, u[:0], u[:0])
    assert lone.max_list == 0 and lone.labels(3).tolist() == [0, 0, 0] and int(lone.counts(3).sum()) == 0


@pytest.mark.parametrize("name,tag", [("cora", "census_cora.npz"), ("citeseer", "census_citeseer.npz")])
def test_cli_writes_the_reference_file(name, tag, tmp_path, monkeypatch):
    g = golden(tag)
    (tmp_path / "preprocess").mkdir()
    (tmp_path / "synthetic_data").mkdir()
    with open(tmp_path / "preprocess" / (name + ".in"), "w") as f:
        f.write("%d %d\n" % (int(g["n"]), len(g["u"])))
        f.write("".join("%d %d\n" % (a, b) for a, b in zip(g["u"], g["v"])))
    monkeypatch.chdir(tmp_path / "synthetic_data")
    assert synth.main([name]) == 0
    out = (tmp_path / "synthetic_data" / (name + "_label.out")).read_bytes()
    assert out == "".join("%d\n" % x for x in g["labels"]).encode()
    assert synth.main([name, "--walk-len", "2"]) == 0
    two = np.array((tmp_path / "synthetic_data" / (name + "_label.out")).read_text().split(), dtype=np.int64)
    assert (two == census_ref.labels_of(census_ref.counts_numpy(int(g["n"]), g["u"], g["v"], 2))).all()
