"""GPU biased walker (pn_sample_paths_biased, MerwSampler.biased) against the CPU restatement tests/biased_ref.py.
Every comparison is exact integer equality of ids, codes and the exhausted count."""
import functools
import math

import numpy as np
import pytest
import torch

import biased_ref
from conftest import golden

pytestmark = pytest.mark.gpu

INF = math.inf
SEED = 0xB1A5ED0123
CORNELL_PQ = [(4, .25), (.25, 4), (INF, 1)]


def dev32(a):
    return torch.as_tensor(np.asarray(a, np.int32)).cuda()


def same(got, want):
    ids, codes = got
    ids, codes = ids.cpu().numpy(), codes.cpu().numpy()
    assert ids.shape == want.ids.shape
    bad = np.argwhere(ids != want.ids)
    assert bad.size == 0, "first id mismatch at %s: got %s want %s" % (bad[0], ids[tuple(bad[0][:-1])],
                                                                       want.ids[tuple(bad[0][:-1])])
    bad = np.argwhere(codes != want.codes)
    assert bad.size == 0, "first code mismatch at %s: got %s want %s" % (bad[0], codes[tuple(bad[0][:-1])],
                                                                         want.codes[tuple(bad[0][:-1])])


@functools.lru_cache(None)
def cornell():
    g = golden("sampler_cornell_7_6.npz")
    return g, biased_ref.merw_tables(int(g["n"]), g["u"], g["v"], g["p"])


@functools.lru_cache(None)
def cornell_sampler(hops):
    from pathnet_amd import MerwSampler
    g, _ = cornell()
    return MerwSampler(int(g["n"]), g["u"], g["v"], g["p"], 6, hops=hops)


@functools.lru_cache(None)
def cornell_ref(p, q):
    """epochs 3 and 4 of the whole graph, W = 7, L = 6: computed once per (p, q), shared, never written to"""
    r = biased_ref.walk(cornell()[1], 7, 6, SEED, p, q, epoch_begin=3, epoch_count=2)
    r.ids.setflags(write=False)
    r.codes.setflags(write=False)
    return r


@pytest.mark.parametrize("p,q", CORNELL_PQ)
def test_cornell_several_workgroups_dense_and_otf(p, q):
    """183 nodes x 7 walks x 2 epochs = 2 562 walks: ten full workgroups of 256 and a partial one"""
    want = cornell_ref(p, q)
    assert want.steps == 2 * 183 * 7 * 5
    got = {}
    for hops in ("dense", "otf"):
        view = cornell_sampler(hops).biased(p, q)
        got[hops] = view.sample(7, SEED, epoch_begin=3, epoch_count=2)
        same(got[hops], want)
        assert view.exhausted_steps() == want.exhausted
    assert torch.equal(got["dense"][0], got["otf"][0]) and torch.equal(got["dense"][1], got["otf"][1])


@pytest.mark.parametrize("hops", ["dense", "otf"])
def test_node_list_gives_those_rows_of_the_full_sample(hops):
    want = cornell_ref(4, .25)
    nodes = [170, 3, 182, 3, 0, 91, 17]                  # unordered, node 3 twice
    view = cornell_sampler(hops).biased(4, .25)
    ids, codes = view.sample(7, SEED, epoch_begin=3, epoch_count=2, nodes=dev32(nodes))
    assert tuple(ids.shape) == (2, len(nodes), 7, 6)
    assert (ids.cpu().numpy() == want.ids[:, nodes]).all() and (codes.cpu().numpy() == want.codes[:, nodes]).all()
    part = biased_ref.walk(cornell()[1], 7, 6, SEED, 4, .25, sources=nodes, epoch_begin=3, epoch_count=2)
    assert (part.ids == want.ids[:, nodes]).all()       # (the restatement agrees that a walk depends on nothing beside it)
    assert view.exhausted_steps() == part.exhausted


def test_out_and_step_state_equal_seed_and_epoch_passed_directly():
    import pathnet_amd
    want = cornell_ref(.25, 4)
    view = cornell_sampler("dense").biased(.25, 4)
    ids = torch.full((1, 183, 7, 6), -1, dtype=torch.int32, device="cuda")
    codes = torch.full((1, 183, 7, 6), 255, dtype=torch.uint8, device="cuda")
    st = pathnet_amd.StepState("cuda", seed=SEED, first_epoch=5)       # (before its first advance: epoch 4, the seed as given)
    assert st.values()["epoch"] == 4 and st.values()["seed"] == SEED
    r = view.sample(7, 0, epoch_begin=0, out=(ids, codes), step_state=st, check=False)     # seed / epoch: the state's
    assert r[0] is ids and r[1] is codes
    assert (ids.cpu().numpy() == want.ids[1:2]).all() and (codes.cpu().numpy() == want.codes[1:2]).all()
    direct = view.sample(7, SEED, epoch_begin=4)
    assert torch.equal(direct[0], ids) and torch.equal(direct[1], codes)
    st.advance()                                                        # epoch 5, the next seed
    now = st.values()
    view.sample(7, 0, out=(ids, codes), step_state=st, check=False)
    direct = view.sample(7, now["seed"], epoch_begin=now["epoch"])
    assert now["epoch"] == 5 and now["seed"] != SEED
    assert torch.equal(direct[0], ids) and torch.equal(direct[1], codes)
    with pytest.raises(ValueError, match="out="):
        view.sample(7, SEED, out=(ids[:, :5], codes[:, :5]))


def test_uniform_tables_and_the_trial_cap_on_cora_nsl():
    """UniformSampler tables on cora_nsl.in (the pair columns of the shipped file, kept in the refbin fixture), (inf, .5):
    never return.  The file lists every pair four times, so a leaf's list is {itself, 4 x its neighbour}: arriving from
    the neighbour, only the self loop (one slot in five, accepted every other time) is no return -- nine trials in ten
    are rejected, and 0.9^63 = 0.13 % of such steps come to the cap (node 999 does, in the walks from 2520), which pins
    the fallback."""
    from pathnet_amd import UniformSampler
    tok = golden("refbin_shipped_cora_nsl.npz")["edge_file"].tobytes().split()
    n, m = int(tok[0]), int(tok[1])
    rows = np.array(tok[2:], dtype=np.float64).reshape(m, -1)
    u, v = rows[:, 0].astype(np.int32), rows[:, 1].astype(np.int32)
    W, L = 2, 4
    want = biased_ref.walk(biased_ref.uniform_tables(n, u, v), W, L, 9, INF, .5)
    assert want.exhausted > 0
    for hops in ("dense", "otf"):
        view = UniformSampler(n, u, v, L, hops=hops).biased(INF, .5)
        same(view.sample(W, 9), want)
        assert view.exhausted_steps() == want.exhausted


@pytest.mark.parametrize("L,hops", [(2, "dense"), (2, "otf"), (8, "otf")])
def test_shortest_and_longest_paths_on_synthetic97(L, hops):
    from pathnet_amd import MerwSampler
    g = golden("sampler_synthetic97_12_5.npz")
    n, W = int(g["n"]), 5
    view = MerwSampler(n, g["u"], g["v"], g["p"], L, hops=hops).biased(3, 7)
    want = biased_ref.walk(biased_ref.merw_tables(n, g["u"], g["v"], g["p"]), W, L, 42, 3, 7, epoch_begin=1)
    same(view.sample(W, 42, epoch_begin=1), want)
    assert view.exhausted_steps() == want.exhausted


def test_index_width_past_2_31_in_the_dense_table():
    """n = 50 000: prev * n + x and source * n + x pass 2^31 from node 46 341 on (dense table: 2.5 GB)"""
    from pathnet_amd import MerwSampler
    n, W, L = 50000, 4, 4
    i = np.arange(n, dtype=np.int64)
    u = np.stack([i, i, i, i], 1).reshape(-1).astype(np.int32)                     # ring both ways, chord, self loop
    v = np.stack([(i + 1) % n, (i - 1) % n, (i * 7919) % n, i], 1).reshape(-1).astype(np.int32)
    p = np.full(len(u), 0.25)
    nodes = [0, 46341, 49999]
    smp = MerwSampler(n, u, v, p, L, hops="dense", build="device")
    for pq in ((.25, 4), (4, .25)):
        view = smp.biased(*pq)
        want = biased_ref.walk(biased_ref.merw_tables(n, u, v, p), W, L, 5, *pq, sources=nodes, epoch_begin=2)
        same(view.sample(W, 5, epoch_begin=2, nodes=dev32(nodes)), want)
        assert view.exhausted_steps() == want.exhausted
        assert want.ids.max() > 46341


@pytest.mark.parametrize("hops", ["dense", "otf"])
def test_empty_table_is_reported_and_the_path_repeats_the_node(hops):
    from pathnet_amd import MerwSampler, _lib
    # (the rows of test_gpu_sampler.py::test_empty_table_is_reported) node 2 has no outgoing rows; walks from 0 reach it
    u = np.array([0, 0, 1, 1], np.int32)
    v = np.array([2, 2, 0, 0], np.int32)
    p = np.array([0.5, 0.5, 0.5, 0.5])
    view = MerwSampler(3, u, v, p, 3, hops=hops).biased(2, .5)
    with pytest.raises(_lib.PnError) as e:
        view.sample(4, 1)
    assert e.value.code == _lib.PN_ERR_EMPTY_TABLE
    want = biased_ref.walk(biased_ref.merw_tables(3, u, v, p), 4, 3, 1, 2, .5)
    assert want.empty
    assert (want.ids[0, 0] == [0, 2, 2]).all() and (want.ids[0, 2] == [2, 2, 2]).all() and (want.ids[0, 1] == [1, 0, 2]).all()
    same(view.sample(4, 1, check=False), want)
    # a walk that ENDS on the empty node needs no table there: no error
    ids, _ = MerwSampler(3, u, v, p, 2, hops=hops).biased(2, .5).sample(4, 1, nodes=dev32([0, 1]))
    assert (ids[0, 0].cpu().numpy() == [0, 2]).all()


@pytest.mark.parametrize("hops", ["dense", "otf"])
def test_codes_equal_annotate(hops):
    view = cornell_sampler(hops).biased(INF, 1)
    ids, codes = view.sample(7, SEED, epoch_begin=3, epoch_count=2)
    again, rep = view.annotate(ids, report=True)
    assert torch.equal(again, codes)
    assert rep.out_of_range == 0 and rep.non_edges == 0 and rep.far == 0          # every step is an edge of the graph
    assert view.n == 183 and view.L == 6 and view.device == cornell_sampler(hops).device


def test_training_loop_takes_the_view(tmp_path):
    from pathnet_amd import MerwSampler, trainer
    from test_gpu_sampler import synthetic_graph
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    n, u, v, p = synthetic_graph(200, 4, 1)
    W, L, F, C = 8, 4, 12, 3
    Y = rng.integers(0, C, n)
    X = rng.random((n, F)).astype(np.float32)
    perm = rng.permutation(n)
    tr, va, te = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    tr[perm[:100]], va[perm[100:150]], te[perm[150:]] = True, True, True
    view = MerwSampler(n, u, v, p, L).biased(2, .5)
    res = trainer.train_fixed_indices(X, Y, C, "synthetic", tr, va, te, W, 32, L, view, epochs=3, save_dir=str(tmp_path))
    assert len(res) == 5 and all(math.isfinite(r) and 0.0 <= r <= 1.0 for r in res)
