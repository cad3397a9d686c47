"""pn_path_codes on the GPU (pn_codes.hip): distance codes and walk checks for paths that did not come from the walker.
Every comparison is exact; the references are the reference program's printed codes (tests/golden), the walker's own
codes, and breadth-first search on the host."""
import numpy as np
import pytest
import torch

from conftest import golden, golden_files

pytestmark = pytest.mark.gpu

HOPS = ("dense", "otf")


def synthetic_graph(n, deg, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n, n * deg // 2)
    b = rng.integers(0, n, n * deg // 2)
    und = np.unique(np.stack([np.minimum(a, b), np.maximum(a, b)], 1)[a != b], axis=0)
    src = np.concatenate([und[:, 0], und[:, 1], np.arange(n)])
    dst = np.concatenate([und[:, 1], und[:, 0], np.arange(n)])
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    w = rng.random(len(src)) + 0.1
    tot = np.zeros(n)
    np.add.at(tot, src, w)
    p = w / tot[src]
    u = np.repeat(src, 2).astype(np.int32)        # every row twice, like the shipped files
    v = np.repeat(dst, 2).astype(np.int32)
    return n, u, v, np.repeat(p, 2)


def hub_and_directed_graph(n, seed):
    """Two hubs with degree > 1100 (their 1- and 2-balls overflow the LDS table, forcing the radius-1 / radius-0
    fallbacks), one-way edges (in-lists != out-lists), a ring."""
    rng = np.random.default_rng(seed)
    src, dst = [], []
    for a in range(n):
        src += [a, a]
        dst += [a, (a + 1) % n]                    # self loop + one-way ring
    for hub in (5, 77):
        leaves = rng.permutation(n)[:1200]
        src += [hub] * len(leaves) + leaves.tolist()
        dst += leaves.tolist() + [hub] * len(leaves)
    extra = rng.integers(0, n, (3 * n, 2))
    src += extra[:, 0].tolist()
    dst += extra[:, 1].tolist()                    # one-way random edges
    src, dst = np.array(src, np.int32), np.array(dst, np.int32)
    key = np.unique(src.astype(np.int64) * n + dst)
    src, dst = (key // n).astype(np.int32), (key % n).astype(np.int32)
    deg = np.bincount(src, minlength=n)
    p = 1.0 / deg[src]
    return n, src, dst, p


ZERO = (0, 0, 0, -1)


# ---- 3. pinned to the reference program ----------------------------------------------------------------------------
@pytest.mark.parametrize("hops", HOPS)
@pytest.mark.parametrize("name", golden_files("sampler_*.npz"))
def test_codes_of_the_reference_programs_paths(name, hops):
    from pathnet_amd import PathAnnotator
    g = golden(name)
    ann = PathAnnotator(int(g["n"]), g["u"], g["v"], int(g["L"]), hops=hops)
    codes, rep = ann.annotate(g["ids"], report=True)
    assert codes.dtype == torch.uint8 and tuple(codes.shape) == g["ids"].shape
    bad = np.argwhere(codes.cpu().numpy() != g["codes"])
    assert bad.size == 0, "first mismatch at %s" % (bad[0],)
    assert tuple(rep) == ZERO, rep


@pytest.mark.parametrize("hops", HOPS)
@pytest.mark.parametrize("name", golden_files("uniform_*.npz"))
def test_codes_of_the_reference_uniform_programs_paths(name, hops):
    from pathnet_amd import UniformSampler
    g = golden(name)
    smp = UniformSampler(int(g["n"]), g["u"], g["v"], int(g["L"]), hops=hops)
    codes, rep = smp.annotate(g["ids"], report=True)
    bad = np.argwhere(codes.cpu().numpy() != g["codes"])
    assert bad.size == 0, "first mismatch at %s" % (bad[0],)
    assert tuple(rep) == ZERO, rep


# ---- 4. round trip: the walker's own paths -------------------------------------------------------------------------
def test_round_trip_at_cora_size_dense():
    from pathnet_amd import DRAW_PHILOX, MerwSampler, PathAnnotator
    n, u, v, p = synthetic_graph(2708, 4, 0)
    smp = MerwSampler(n, u, v, p, 4, hops="dense")
    ids, codes = smp.sample(40, 11, epoch_count=2, draw_source=DRAW_PHILOX)
    got, rep = smp.annotate(ids, report=True)
    assert torch.equal(got, codes) and tuple(rep) == ZERO
    for build in ("host", "device"):            # the stand-alone hop source, both builders
        got, rep = PathAnnotator(n, u, v, 4, hops="dense", build=build).annotate(ids, report=True)
        assert torch.equal(got, codes) and tuple(rep) == ZERO, build
    got, rep = PathAnnotator(n, u, v, 4, hops="otf", build="device").annotate(ids, report=True)
    assert torch.equal(got, codes) and tuple(rep) == ZERO      # (the edge check searches the device-built sorted lists)


def test_round_trip_on_the_large_graph_on_the_fly():
    from pathnet_amd import DRAW_PHILOX, MerwSampler
    n, u, v, p = synthetic_graph(400000, 8, 12)
    smp = MerwSampler(n, u, v, p, 6, hops="auto")
    assert smp.hops == "otf"
    ids, codes = smp.sample(40, 5, node_begin=1234, node_count=2000, draw_source=DRAW_PHILOX)
    got, rep = smp.annotate(ids, report=True)
    bad = torch.nonzero(got != codes)
    assert bad.numel() == 0, "first mismatch %s" % (bad[0].tolist(),)
    assert tuple(rep) == ZERO, rep


@pytest.mark.parametrize("hops", HOPS)
@pytest.mark.parametrize("L", [3, 4, 6, 8])
def test_round_trip_on_hubs_and_directed_edges(L, hops):
    from pathnet_amd import DRAW_PHILOX, MerwSampler
    n, u, v, p = hub_and_directed_graph(4000, 9)
    smp = MerwSampler(n, u, v, p, L, hops=hops)
    ids, codes = smp.sample(6, 77, epoch_count=2, draw_source=DRAW_PHILOX)
    got, rep = smp.annotate(ids, report=True)
    bad = torch.nonzero(got != codes)
    assert bad.numel() == 0, "first mismatch %s: walker %d annotator %d" % (
        bad[0].tolist(), int(codes[tuple(bad[0])]), int(got[tuple(bad[0])]))
    assert tuple(rep) == ZERO, rep


# ---- 5. paths that are not walks -----------------------------------------------------------------------------------
@pytest.mark.parametrize("hops", HOPS)
@pytest.mark.parametrize("L", [1, 2, 4, 8])
def test_arbitrary_targets_match_breadth_first_search(L, hops):
    """Random ids, random sources -- among them both hubs (radius-0 fallback), a leaf of each (radius 1) and a node whose
    2-ball fits the table: every code is min(BFS hops, L-1), `far` and `non_edges` are the counts the same BFS gives.
    L = 1 and 2 are shorter than the ball's radius: a node on the ball's outer levels is then far, not its level."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import dijkstra
    from pathnet_amd import PathAnnotator
    n, u, v, _ = hub_and_directed_graph(4000, 9)
    rng = np.random.default_rng(100 + L)
    S, W = 96, 5
    ids = rng.integers(0, n, (S, W, L)).astype(np.int32)
    sources = rng.integers(0, n, S).astype(np.int32)
    out_deg = np.bincount(u, minlength=n)
    leaves = [int(next(b for a, b in zip(u, v) if a == hub and b != hub and out_deg[b] < 100)) for hub in (5, 77)]
    two_ball = lambda s: 1 + out_deg[s] + int(out_deg[v[u == s]].sum())      # noqa: E731  (an upper bound of its size)
    small = int(next(s for s in range(100, n) if two_ball(s) < 200))
    sources[:5] = (5, 77, leaves[0], leaves[1], small)
    one = np.setdiff1d(v[u == small], [small])                # the small ball's level 1 and level 2
    two = np.setdiff1d(v[np.isin(u, one)], np.append(one, small))
    assert len(one) and len(two)
    ids[4, 0], ids[4, 1] = np.resize(one, L), np.resize(two, L)
    assert out_deg[5] > 1024 and out_deg[77] > 1024          # more out-neighbours than the LDS table takes
    ids[0, 0, :min(L, 3)] = (5, leaves[0], 5)[:L]             # a few real steps among the random ones
    A = sp.csr_matrix((np.ones(len(u), np.int8), (u, v)), shape=(n, n))
    dist = dijkstra(A, unweighted=True, indices=sources, limit=L)        # inf beyond L hops
    d = dist[np.arange(S)[:, None, None], ids]
    want = np.minimum(d, L - 1).astype(np.uint8)
    far = int((d > L - 1).sum())
    edge = set((u.astype(np.int64) * n + v).tolist())
    a, b = ids[..., :-1].astype(np.int64), ids[..., 1:].astype(np.int64)
    non_edges = int(sum(1 for x, y in zip(a.ravel().tolist(), b.ravel().tolist()) if x != y and x * n + y not in edge))
    ann = PathAnnotator(n, u, v, L, hops=hops)
    codes, rep = ann.annotate(torch.from_numpy(ids).cuda(), torch.from_numpy(sources).cuda(), report=True)
    got = codes.cpu().numpy()
    print("L=%d %s: far %d (want %d) non_edges %d (want %d) mismatches %d" % (
        L, hops, rep.far, far, rep.non_edges, non_edges, int((got != want).sum())))
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first mismatch at %s (source %d, node %d): got %d want %d" % (
        bad[0], sources[bad[0][0]], ids[tuple(bad[0])], got[tuple(bad[0])], want[tuple(bad[0])])
    assert (rep.out_of_range, rep.first_bad) == (0, -1)
    assert rep.far == far and rep.non_edges == non_edges


# ---- 6. planted faults ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hops", HOPS)
def test_planted_ids_outside_the_graph_are_counted_and_touch_nothing_else(hops):
    from pathnet_amd import DRAW_PHILOX, MerwSampler
    n, u, v, p = hub_and_directed_graph(4000, 9)
    L, W = 4, 8
    smp = MerwSampler(n, u, v, p, L, hops=hops)
    ids, _ = smp.sample(W, 3, node_begin=100, node_count=50, draw_source=DRAW_PHILOX)
    ids = ids[0]
    clean, rep = smp.annotate(ids, report=True)
    assert tuple(rep) == ZERO
    planted = {(3, 2, 1): -1, (10, 0, 3): n, (10, 5, 2): 2 ** 31 - 1, (49, 7, 3): -(2 ** 31)}
    bad_ids = ids.clone()
    for at, val in planted.items():
        bad_ids[at] = val
    codes, rep = smp.annotate(bad_ids, report=True)
    torch.cuda.synchronize()                                  # a clean return: nothing faulted
    assert rep.out_of_range == len(planted)
    assert rep.first_bad == (3 * W + 2) * L + 1
    assert rep.non_edges == 0 and rep.far == 0               # a step with an id outside the graph is not judged
    hit = torch.zeros_like(ids, dtype=torch.bool)
    for at in planted:
        hit[at] = True
    assert (codes[hit] == L - 1).all()
    assert torch.equal(codes[~hit], clean[~hit])
    with pytest.raises(IndexError, match="element %d " % ((3 * W + 2) * L + 1)):
        smp.annotate(bad_ids, check=True)
    assert torch.equal(smp.annotate(ids, check=True), clean)
    # a wider dtype on the host is narrowed without wrapping into the graph
    wide = bad_ids.cpu().to(torch.int64)
    wide[10, 5, 2] = 2 ** 32 + 7
    c2, r2 = smp.annotate(wide.numpy(), report=True)
    assert torch.equal(c2, codes) and tuple(r2) == tuple(rep)


# ---- 7. sources given ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hops", HOPS)
def test_reversed_paths_with_their_sources_given(hops):
    from pathnet_amd import DRAW_PHILOX, MerwSampler
    n, u, v, p = hub_and_directed_graph(4000, 9)
    smp = MerwSampler(n, u, v, p, 6, hops=hops)
    ids, codes = smp.sample(7, 21, node_count=300, draw_source=DRAW_PHILOX)
    ids, codes = ids[0], codes[0]
    assert torch.equal(smp.annotate(ids), codes)
    flipped = smp.annotate(ids.flip(-1).contiguous(), sources=ids[:, 0, 0].contiguous())
    assert torch.equal(flipped, codes.flip(-1))
    out = torch.empty_like(codes)
    assert smp.annotate(ids.flip(-1).contiguous(), ids[:, 0, 0].cpu().numpy(), out=out) is out
    assert torch.equal(out, codes.flip(-1))


# ---- 8. stream use -------------------------------------------------------------------------------------------------
def test_annotate_on_a_side_stream_and_into_an_aggregator():
    import pathnet_amd
    from pathnet_amd import DRAW_PHILOX, MerwSampler
    n, u, v, p = synthetic_graph(2708, 4, 0)
    W, L, S, F, H, C = 8, 4, 200, 24, 64, 5
    smp = MerwSampler(n, u, v, p, L)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ids, codes = smp.sample(W, 9, node_count=S, draw_source=DRAW_PHILOX, check=False)
        on_side = smp.annotate(ids)                         # no flag: nothing is read back
    side.synchronize()
    assert torch.equal(on_side, codes)
    assert torch.equal(smp.annotate(ids), on_side)
    torch.manual_seed(0)
    model = pathnet_amd.PathNet_homo(F, H, C, L).cuda().eval()
    X = torch.rand(n, F).cuda()
    sel = torch.arange(S, dtype=torch.int32)
    with torch.no_grad():
        a = model(X, ids[0], W, L, sel, codes[0], None)
        b = model(X, ids[0], W, L, sel, on_side[0], None)
    assert torch.equal(a, b)
