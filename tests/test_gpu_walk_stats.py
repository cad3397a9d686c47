"""GPU walk statistics (pn_walk_stats, pathnet_amd.walk_stats) against the NumPy restatement tests/walk_stats_ref.py.
Every comparison is exact integer equality."""
import functools

import numpy as np
import pytest
import torch

import walk_stats_ref as ref
from conftest import golden, golden_files

pytestmark = pytest.mark.gpu

FIELDS = ref.FIELDS
INT_MAX = 2 ** 31 - 1


def labels_for(n, C=5):
    node = np.arange(n, dtype=np.int64)
    lab = ((node * 2654435761) >> 7) % C
    lab[::11] = -1
    return lab.astype(np.int32)


def run(ids, codes, n, **kw):
    from pathnet_amd import walk_stats
    for k in ("labels", "sources"):
        if kw.get(k) is not None:
            kw[k] = torch.as_tensor(np.array(kw[k], np.int32)).cuda()
    return walk_stats(torch.as_tensor(np.array(ids, np.int32)).cuda(), torch.as_tensor(np.array(codes, np.uint8)).cuda(), n,
                      **kw)


def same(got, want, fields=FIELDS):
    for f in fields:
        g, w = getattr(got, f), getattr(want, f)
        if w is None:
            assert g is None, f
            continue
        assert g is not None, f
        g = g.cpu().numpy()
        assert g.dtype == w.dtype, (f, g.dtype)
        g = g.reshape(w.shape) if f in ("unique_paths", "cover") else g
        assert g.shape == w.shape, (f, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.size == 0, "%s: first mismatch at %s: got %s want %s (%d wrong)" % (
            f, bad[0], g[tuple(bad[0])], w[tuple(bad[0])], len(bad))


def random_paths(seed, rows, W, L, n, spread=None):
    """ids drawn from `spread` ids (default n) so that repeated nodes and repeated paths are common; every path of a row
    starts at the row's source; codes anywhere in [0, L)"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, spread or n, size=(rows, W, L)).astype(np.int32)
    if rows:
        ids[:, :, 0] = ids[:, :1, 0]
    codes = rng.integers(0, L, size=(rows, W, L)).astype(np.uint8)
    return ids, codes


def both(ids, codes, n, **kw):
    """(GPU result with every output, restatement)"""
    got = run(ids, codes, n, visits=True, **kw)
    want = ref.walk_stats(ids, codes, n, labels=kw.get("labels"), num_classes=kw.get("num_classes"),
                          sources=kw.get("sources"))
    same(got, want)
    return got, want


# ---- the goldens -----------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def golden_case(name):
    """-> (ids, codes, n, labels, restatement): computed once, shared, never written to"""
    g = golden(name)
    n = int(g["n"])
    lab = labels_for(n)
    want = ref.walk_stats(g["ids"], g["codes"], n, labels=lab, num_classes=5)
    for a in (g["ids"], g["codes"], lab) + tuple(x for x in want if x is not None):
        a.setflags(write=False)
    return g["ids"], g["codes"], n, lab, want


@pytest.mark.parametrize("name", golden_files("sampler_*.npz"))
def test_every_output_on_the_sampler_goldens(name):
    """W = 40, 10, 7, 12, 5 and L = 4, 6, 5; Cora's 2 708 rows are several rounds of several workgroups"""
    ids, codes, n, lab, want = golden_case(name)
    got = run(ids, codes, n, labels=lab, num_classes=5, visits=True)
    same(got, want)
    assert tuple(got.unique_paths.shape) == ids.shape[:-2] == tuple(got.cover.shape)
    s = got.summary()
    assert s["step_code"] == want.step_code.tolist() and s["paths"] == ids.size // ids.shape[-1]
    assert s["mean_cover"] == float(want.cover.sum()) / want.cover.size
    assert s["out_of_range"] == 0 and s["bad_codes"] == 0 and s["visits"] == int(want.visits.sum())


# ---- edges of the shape ----------------------------------------------------------------------------------------------

SHAPES = [  # rows, W, L, n, spread, C
    (7, 1, 1, 9, None, 5),            # one entry per row
    (6, 9, 2, 4, None, 5),            # L = 2: no step can turn back
    (5, 65, 4, 50, 3, 5),             # one path past a wavefront
    (9, 256, 4, 300, 5, 5),           # W * L = 1024: the last shape a wavefront takes
    (5, 1025, 1, 2000, None, 5),      # W * L = 1025: the first shape a workgroup takes
    (3, 1024, 8, 5000, 3, 5),         # W * L at its limit
    (2, 8192, 1, 6000, None, 5),      # W at its limit: the longest index sort
    (5, 11, 16, 40, None, 64),        # L = 16, C = 64: the largest tables (label_pairs counted with global atomics)
    (6, 13, 4, 60, None, 22),         # L * C * C = 1936: the largest label_pairs counted in LDS ...
    (6, 13, 4, 60, None, 23),         # ... and 2116, the first that is not
    (6, 13, 5, 60, None, 1),          # one class
    (0, 7, 4, 10, None, 5),           # no rows
    (8198, 2, 3, 30, 4, 5),           # 2 050 workgroups' worth of rows on a grid of 2 048: a second round, idle row slots
]


@pytest.mark.parametrize("rows,W,L,n,spread,C", SHAPES)
def test_shape_edges(rows, W, L, n, spread, C):
    ids, codes = random_paths(rows * 131 + W, rows, W, L, n, spread)
    got, want = both(ids, codes, n, labels=labels_for(n, C), num_classes=C)
    if L == 2:
        assert int(got.back.sum()) == 0
    if rows == 0:
        assert all(int(getattr(got, f).sum()) == 0 for f in ref.GLOBAL)
        assert got.unique_paths.numel() == 0 and got.cover.numel() == 0


# ---- content ---------------------------------------------------------------------------------------------------------

def test_identical_paths_and_identical_entries():
    ids = np.tile(np.array([3, 5, 3, 8, 5], np.int32), (4, 70, 1))
    codes = np.tile(np.array([0, 1, 0, 2, 1], np.uint8), (4, 70, 1))
    got, _ = both(ids, codes, 9)
    assert got.unique_paths.tolist() == [1] * 4 and got.cover.tolist() == [3] * 4
    ids[:] = 7
    got, _ = both(ids, codes, 9)
    assert got.unique_paths.tolist() == [1] * 4 and got.cover.tolist() == [1] * 4
    assert got.distinct_hist.tolist() == [0, 280, 0, 0, 0, 0]


def test_paths_that_differ_in_one_place_only():
    # every path distinct, differing only in the last node
    W, L = 70, 5
    ids = np.tile(np.array([5, 6, 7, 8, 0], np.int32), (3, W, 1))
    ids[:, :, 4] = 100 + np.arange(W)[::-1]
    codes = np.tile(np.array([0, 1, 2, 3, 4], np.uint8), (3, W, 1))
    got, _ = both(ids, codes, 200)
    assert got.unique_paths.tolist() == [W] * 3 and got.cover.tolist() == [4 + W] * 3
    # two paths that differ only in the first step after the source, among copies of both
    ids = np.array([[[1, 2, 3, 4], [1, 9, 3, 4], [1, 2, 3, 4], [1, 9, 3, 4], [1, 9, 3, 4]]], np.int32)
    codes = np.zeros(ids.shape, np.uint8)
    got, _ = both(ids, codes, 10)
    assert got.unique_paths.tolist() == [2] and got.cover.tolist() == [5]


def test_ids_outside_the_graph_and_codes_beyond_L():
    n, C = 40, 5
    ids, codes = random_paths(5, 12, 33, 6, n, spread=6)
    rng = np.random.default_rng(6)
    for v in (-1, n, INT_MAX, -2 ** 31, n + 1):
        ids[rng.integers(0, 12, 40), rng.integers(0, 33, 40), rng.integers(0, 6, 40)] = v
    ids[3] = INT_MAX                    # a whole row outside the graph, its source included
    ids[4, :, 0] = 7
    ids[4, :, 1:] = -1
    codes[rng.integers(0, 12, 60), rng.integers(0, 33, 60), rng.integers(0, 6, 60)] = rng.integers(6, 256, 60)
    codes[5, 2] = 255
    got, want = both(ids, codes, n, labels=labels_for(n, C), num_classes=C)
    assert want.counters[0] > 33 * 6 and want.counters[1] > 6
    assert got.cover[3].item() == 1 and got.cover[4].item() == 2


def test_sources_given_some_outside_the_graph():
    n, C = 40, 5
    ids, codes = random_paths(8, 10, 9, 4, n)
    sources = np.array([0, 39, -1, n, INT_MAX, 11, 22, 5, 5, 17], np.int32)       # 0, 11 and 22 are unlabelled
    got, want = both(ids, codes, n, labels=labels_for(n, C), num_classes=C, sources=sources)
    plain = ref.walk_stats(ids, codes, n, labels=labels_for(n, C), num_classes=C)
    assert (want.unlabeled > plain.unlabeled).any() and want.counters.tolist() == plain.counters.tolist()


# ---- outputs that are not wanted ---------------------------------------------------------------------------------------

def cornell():
    return golden_case("sampler_cornell_40_4.npz")


def test_each_output_can_be_left_out():
    from pathnet_amd import WalkStats
    ids, codes, n, lab, want = cornell()
    for f in FIELDS:
        bufs = run(ids, codes, n, labels=lab, num_classes=5, visits=True)
        for t in bufs:
            t.fill_(-7)
        got = run(ids, codes, n, labels=lab, num_classes=5, out=bufs._replace(**{f: None}))
        assert getattr(got, f) is None and bool((getattr(bufs, f) == -7).all())      # left alone
        same(got, want, [k for k in FIELDS if k != f])
        assert all(a is b for a, b in zip(got, bufs._replace(**{f: None})))
    with pytest.raises(ValueError):
        run(ids, codes, n, out=WalkStats(*bufs))          # label tables without labels


def test_without_labels_the_label_tables_are_not_produced():
    ids, codes, n, lab, want = cornell()
    got = run(ids, codes, n)
    assert got.label_pairs is None and got.unlabeled is None and got.visits is None
    same(got, want, [f for f in FIELDS if f not in ("label_pairs", "unlabeled", "visits")])
    got = run(ids, codes, n, per_row=False)
    assert got.unique_paths is None and got.cover is None
    same(got, want, ["step_code", "stay", "back", "distinct_hist", "counters"])


def test_nothing_is_written_around_the_outputs():
    from pathnet_amd import WalkStats
    ids, codes, n, lab, want = cornell()
    C, L, pad = 5, 4, 37
    bufs, views = {}, {}
    for f in FIELDS:
        w = getattr(want, f)
        dt, sentinel = (torch.int32, -0x5A5A5A5B) if w.dtype == np.int32 else (torch.int64, -0x5A5A5A5A5A5A5A5B)
        bufs[f] = torch.full((w.size + 2 * pad,), sentinel, dtype=dt, device="cuda")
        views[f] = bufs[f][pad:pad + w.size].view(w.shape if f not in ("unique_paths", "cover") else ids.shape[:-2])
    got = run(ids, codes, n, labels=lab, num_classes=C, out=WalkStats(**views))
    same(got, want)
    for f in FIELDS:
        b = bufs[f].cpu()
        guard = torch.cat((b[:pad], b[-pad:]))
        assert bool((guard == guard[0]).all()) and guard[0].item() < 0, f


# ---- accumulate, streams ---------------------------------------------------------------------------------------------

def test_two_halves_accumulated_equal_one_call():
    ids, codes, n, lab, want = cornell()
    first = run(ids[:1], codes[:1], n, labels=lab, num_classes=5, visits=True)
    total = run(ids[1:], codes[1:], n, labels=lab, num_classes=5, accumulate_into=first)
    same(total, want, ref.GLOBAL)
    assert all(getattr(total, f) is getattr(first, f) for f in ref.GLOBAL)
    assert (total.cover.cpu().numpy() == want.cover.reshape(2, -1)[1:]).all()
    assert (total.unique_paths.cpu().numpy() == want.unique_paths.reshape(2, -1)[1:]).all()
    # a plain call over the same buffers starts from zero again
    again = run(ids, codes, n, labels=lab, num_classes=5, out=total._replace(unique_paths=None, cover=None))
    same(again, want, ref.GLOBAL)


def test_on_a_side_stream():
    ids, codes, n, lab, want = cornell()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = run(ids, codes, n, labels=lab, num_classes=5, visits=True)
    s.synchronize()
    same(got, want)


# ---- with the walkers --------------------------------------------------------------------------------------------------

def test_a_non_backtracking_walk_never_turns_back():
    from pathnet_amd import MerwSampler
    n = 41
    u, v = [], []
    for i in range(n):
        for d in (1, 5, 12):            # the ring and two chords, both directions, no self loops
            u += [i, i]
            v += [(i + d) % n, (i - d) % n]
    u, v = np.array(u, np.int32), np.array(v, np.int32)
    smp = MerwSampler(n, u, v, np.full(len(u), 1.0 / 6), 6)
    view = smp.biased(float("inf"), 1.0)
    ids, codes = view.sample(20, 12345, epoch_count=3)
    assert view.exhausted_steps() == 0
    st = view.walk_stats(ids, codes)
    assert int(st.back.sum()) == 0 and int(st.stay.sum()) == 0
    plain = smp.walk_stats(*smp.sample(20, 12345, epoch_count=3))
    assert int(plain.back.sum()) > 0        # the plain walk over the same tables does turn back
    same(st, ref.walk_stats(ids.cpu().numpy(), codes.cpu().numpy(), n), ["step_code", "back", "stay", "unique_paths"])


@pytest.mark.parametrize("hops", ["dense", "otf"])
def test_sampler_method_in_both_hop_modes(hops):
    from pathnet_amd import MerwSampler
    g = golden("sampler_cornell_7_6.npz")
    smp = MerwSampler(int(g["n"]), g["u"], g["v"], g["p"], 6, hops=hops)
    ids, codes = smp.sample(7, 99, epoch_count=2)
    got = smp.walk_stats(ids, codes, visits=True)
    same(got, ref.walk_stats(ids.cpu().numpy(), codes.cpu().numpy(), smp.n))


def test_command_line_prints_one_json_object(tmp_path, capsys):
    """in-process (main()): three epochs in one run equal the restatement over the same Philox paths, with and without a bias"""
    import json
    import os

    from oracle import merw
    from pathnet_amd import MerwSampler, walkstats
    g = golden("sampler_cornell_7_6.npz")
    n = int(g["n"])
    edge = os.path.join(tmp_path, "cornell.in")
    merw.write_edge_file(edge, n, g["u"], g["v"], g["p"])
    lab = labels_for(n)
    np.savetxt(os.path.join(tmp_path, "labels.txt"), lab, fmt="%d")
    smp = MerwSampler(n, g["u"], g["v"], g["p"], 5)
    for bias in (None, "4,0.25"):
        argv = [edge, "9", "5", "--epochs", "3", "--seed", "77", "--labels", os.path.join(tmp_path, "labels.txt")]
        assert walkstats.main(argv + (["--bias", bias] if bias else [])) == 0
        out = capsys.readouterr().out.strip().splitlines()
        assert len(out) == 1
        res = json.loads(out[0])
        view = smp.biased(4, .25) if bias else smp
        ids, codes = view.sample(9, 77, epoch_count=3)
        want = ref.walk_stats(ids.cpu().numpy(), codes.cpu().numpy(), n, labels=lab, num_classes=5)
        assert res["step_code"] == want.step_code.tolist() and res["n"] == n and res["epochs"] == 3
        paths = 3 * n * 9
        assert res["stay_share"] == [float(x) / paths for x in want.stay] and res["back_share"] == [float(x) / paths for x in want.back]
        assert res["mean_unique_paths"] == float(want.unique_paths.sum()) / (3 * n)
        assert res["mean_cover"] == float(want.cover.sum()) / (3 * n)
        agree = [float(np.trace(m)) / float(m.sum()) if m.sum() else None for m in want.label_pairs]
        assert res["label_agreement"] == agree and res["unlabeled"] == want.unlabeled.tolist()
