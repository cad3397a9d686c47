"""The sampler's tables built on the GPU (pn_tables.hip, MerwSampler(build="device")) against the host builders, bit
for bit: alias triples, node_ref, the fp64 splits (as int64 views), both CSR lists and the dense hop table; then walks
from device-built samplers against the reference-binary goldens and host-built samplers."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import golden, golden_files
from pathnet_amd import DRAW_GLIBC_REPLAY, DRAW_PHILOX, MerwSampler, _lib, sampler

pytestmark = pytest.mark.gpu


def host_alias(n, u, v, p):
    """build_alias -> pn_alias_pack / pn_node_ref_pack, as MerwSampler(build="host") does"""
    lib = _lib.load()
    off, A, B, S, thr = sampler.build_alias(n, u, v, p)
    packed = np.zeros(max(len(A), 1) * 4, np.int32)
    _lib.check(lib.pn_alias_pack(len(A), _lib.np_ptr(A, ctypes.c_int32), _lib.np_ptr(B, ctypes.c_int32),
                                 _lib.np_ptr(thr, ctypes.c_uint32), _lib.np_ptr(packed, ctypes.c_int32)))
    ref = np.zeros(2 * max(n, 1), np.uint32)
    _lib.check(lib.pn_node_ref_pack(n, _lib.np_ptr(off, ctypes.c_int64), _lib.np_ptr(ref, ctypes.c_uint32)))
    return off, packed, ref, S


def check_alias(n, u, v, p):
    off, packed, ref, S = host_alias(n, u, v, p)
    d_off, d_packed, d_ref, d_S = sampler.build_alias_device(n, u, v, p, split=True)
    t = len(S)
    assert np.array_equal(d_off.cpu().numpy(), off)
    got = d_packed.cpu().numpy()[:4 * t]
    bad = np.argwhere(got != packed[:4 * t])
    assert bad.size == 0, "triple word %d: got %d want %d" % (bad[0][0], got[bad[0][0]], packed[bad[0][0]])
    assert np.array_equal(d_ref.cpu().numpy().view(np.uint32)[:2 * n], ref[:2 * n])
    assert np.array_equal(d_S.cpu().numpy().view(np.int64), S.view(np.int64))
    return off, packed, S


@pytest.mark.parametrize("name", golden_files("sampler_*.npz"))
def test_alias_tables_match_host_on_goldens(name):
    g = golden(name)
    check_alias(int(g["n"]), g["u"], g["v"], g["p"])


def random_rows(rng, n, m, self_loops=True):
    u = rng.integers(0, n, m).astype(np.int32)
    v = rng.integers(0, n, m).astype(np.int32)
    if not self_loops:
        v = np.where(u == v, (v + 1) % n, v).astype(np.int32)
    return u, v


def test_alias_shuffled_rows_duplicates_self_loops_and_empty_nodes():
    rng = np.random.default_rng(1)
    n = 300
    u, v = random_rows(rng, n // 2, 4000)
    u, v = u * 2, np.concatenate([v[:2000], u[:2000]]) * 2 + 1     # even sources only: the odd nodes have no rows
    u[:50] = v[:50] = 4                             # a self loop, fifty times
    u[50:80], v[50:80] = 6, 9                       # one duplicated pair
    p = rng.random(len(u))
    p /= np.bincount(u, p, minlength=n)[u]          # MERW-like: the rows of a node sum to 1
    perm = rng.permutation(len(u))                  # file order: not sorted by source
    off, _, _ = check_alias(n, u[perm], v[perm].astype(np.int32), p[perm])
    assert (np.diff(off)[1::2] == 0).all()


def test_alias_non_finite_zero_and_negative_probabilities():
    rng = np.random.default_rng(2)
    n = 64
    u, v = random_rows(rng, n, 1500)
    p = rng.random(len(u)) * 2 - 0.5
    specials = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, 1e300, 5e-324, 2.5])
    p[rng.choice(len(u), 200, replace=False)] = rng.choice(specials, 200)
    check_alias(n, u, v, p)


def test_alias_extra_triple_branch():
    """masses whose pair step leaves |rest - 1| < 1e-5: the extra (hv, hv, rest) triple of gen_merw.cpp:48"""
    rng = np.random.default_rng(3)
    us, vs, ps = [], [], []
    for node in range(200):
        k = int(rng.integers(2, 9))
        mass = rng.random(k) + 0.1
        # a heavy item h and a light item l with h + l = 2 + tiny: rest = h - (1 - l) lands next to 1
        mass[0] = 1.0 + rng.random() * 0.8
        mass[1] = 2.0 - mass[0] + rng.choice([0.0, 3e-6, -7e-6, 9.9e-6, 2e-5])
        us += [node] * k
        vs += list(rng.integers(0, 200, k))
        ps += list(mass / k)
    u, v, p = np.array(us, np.int32), np.array(vs, np.int32), np.array(ps)
    off, packed, S = check_alias(200, u, v, p)
    A, B = packed[0::4][:len(S)], packed[1::4][:len(S)]
    assert ((A == B) & (S != 1.0)).sum() >= 50     # the branch was taken, and often


def test_alias_power_law_hub():
    rng = np.random.default_rng(4)
    n, hub = 5000, 120_000
    u = np.concatenate([np.full(hub, 17, np.int32), rng.integers(0, n, 20_000).astype(np.int32)])
    v = rng.integers(0, n, len(u)).astype(np.int32)
    p = rng.random(len(u))
    p /= np.bincount(u, p, minlength=n)[u]
    perm = rng.permutation(len(u))
    off, _, _ = check_alias(n, u[perm], v[perm], p[perm])
    assert off[18] - off[17] >= 100_000


@pytest.mark.parametrize("n", [0, 1])
def test_alias_tiny_graphs(n):
    e = np.zeros(0, np.int32)
    check_alias(n, e, e, np.zeros(0))
    if n:
        check_alias(n, np.zeros(3, np.int32), np.zeros(3, np.int32), np.array([0.5, 0.25, 0.25]))


def check_csr_and_hops(n, u, v, Ls):
    for rev in (False, True):
        off, adj = sampler.csr_build(n, u, v, reverse=rev)
        d_off, d_adj = sampler.csr_build_device(n, u, v, reverse=rev)
        assert np.array_equal(d_off.cpu().numpy(), off) and np.array_equal(d_adj.cpu().numpy(), adj)
    d_off, d_adj = sampler.csr_build_device(n, u, v)
    for L in Ls:
        dis = sampler.hops_dense_device(n, d_off, d_adj, L).cpu().numpy()
        want = sampler.hops_dense(n, u, v, L)
        bad = np.argwhere(dis != want)
        assert bad.size == 0, "L=%d dis%s: got %d want %d" % (L, bad[0], dis[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("name", golden_files("sampler_*.npz"))
def test_csr_and_dense_hops_match_host_on_goldens(name):
    g = golden(name)
    check_csr_and_hops(int(g["n"]), g["u"], g["v"], [int(g["L"]), 2, 8])


def test_csr_and_dense_hops_directed_one_way_edges():
    rng = np.random.default_rng(5)
    n = 700
    u, v = random_rows(rng, n, 2100, self_loops=False)          # a sparse directed graph: most edges one way
    u = np.concatenate([u, u[:300]])                            # repeated rows
    v = np.concatenate([v, v[:300]])
    perm = rng.permutation(len(u))
    check_csr_and_hops(n, u[perm], v[perm], range(2, 9))
    check_csr_and_hops(1, np.zeros(0, np.int32), np.zeros(0, np.int32), [1, 4])
    check_csr_and_hops(5, np.zeros(0, np.int32), np.zeros(0, np.int32), [1, 4])


def host_error(fn):
    with pytest.raises(_lib.PnError) as e:
        fn()
    return e.value


@pytest.mark.parametrize("bad", ["source", "target", "negative"])
def test_out_of_range_rows_name_the_host_row(bad):
    rng = np.random.default_rng(6)
    n = 50
    u, v = random_rows(rng, n, 400)
    p = np.full(len(u), 0.1)
    if bad == "source":
        u[123], v[200] = n, n + 5
    elif bad == "target":
        v[77], u[301] = n, -1
    else:
        u[9], v[8] = -3, -2**31
    for host, dev in ((lambda: sampler.build_alias(n, u, v, p), lambda: sampler.build_alias_device(n, u, v, p)),
                      (lambda: sampler.csr_build(n, u, v), lambda: sampler.csr_build_device(n, u, v)),
                      (lambda: sampler.csr_build(n, u, v, True), lambda: sampler.csr_build_device(n, u, v, True))):
        h, d = host_error(host), host_error(dev)
        assert h.code == d.code == _lib.PN_ERR_ARG
        hm, dm = re.search(r"edge row \d+.*", str(h)).group(0), re.search(r"edge row \d+.*", str(d)).group(0)
        assert hm == dm


def test_short_capacity_and_bad_seq_len():
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    g = golden("sampler_cornell_40_4.npz")
    n = int(g["n"])
    u = torch.from_numpy(g["u"]).to(dev)
    v = torch.from_numpy(g["v"]).to(dev)
    p = torch.from_numpy(g["p"]).to(dev)
    m = u.numel()
    ws = sampler.tables_workspace(n, m, dev)
    off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    buf = torch.empty(4 * m, dtype=torch.int32, device=dev)
    cnt = ctypes.c_int64(0)
    st = _lib.stream_ptr(dev)
    P = _lib.ptr
    # sizing call, then one triple short
    _lib.check(lib.pn_alias_build_device(n, m, P(u), P(v), P(p), P(off), None, None, None, 0, ctypes.byref(cnt), P(ws),
                                         ws.numel(), st))
    assert cnt.value == m
    assert np.array_equal(off.cpu().numpy(), sampler.build_alias(n, g["u"], g["v"], g["p"])[0])
    assert lib.pn_alias_build_device(n, m, P(u), P(v), P(p), P(off), P(buf), None, None, m - 1, ctypes.byref(cnt),
                                     P(ws), ws.numel(), st) == _lib.PN_ERR_CAPACITY
    assert lib.pn_alias_build_device(n, m, P(u), P(v), P(p), P(off), P(buf), None, None, m, ctypes.byref(cnt),
                                     P(ws), 1024, st) == _lib.PN_ERR_CAPACITY
    _lib.check(lib.pn_csr_build_device(n, m, P(u), P(v), 0, P(off), None, 0, ctypes.byref(cnt), P(ws), ws.numel(), st))
    assert cnt.value == len(sampler.csr_build(n, g["u"], g["v"])[1])
    assert lib.pn_csr_build_device(n, m, P(u), P(v), 0, P(off), P(buf), cnt.value - 1, ctypes.byref(cnt), P(ws),
                                   ws.numel(), st) == _lib.PN_ERR_CAPACITY
    d_off, d_adj = sampler.csr_build_device(n, u, v)
    for L in (0, 255):
        with pytest.raises(_lib.PnError) as e:
            sampler.hops_dense_device(n, d_off, d_adj, L)
        assert e.value.code == _lib.PN_ERR_ARG
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", golden_files("sampler_*.npz"))
def test_device_built_sampler_glibc_replay_bit_exact_vs_reference_golden(name):
    g = golden(name)
    smp = MerwSampler(int(g["n"]), g["u"], g["v"], g["p"], int(g["L"]), build="device")
    assert smp.host is None
    ids, codes = smp.sample(int(g["W"]), int(g["seed"]), epoch_count=int(g["epochs"]), draw_source=DRAW_GLIBC_REPLAY)
    assert np.array_equal(ids.cpu().numpy(), g["ids"]) and np.array_equal(codes.cpu().numpy(), g["codes"])


def same_tables(a, b):
    for k in ("d_off", "d_triples", "d_node_ref", "d_dis", "d_adj_off", "d_adj", "d_radj_off", "d_radj"):
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None), k
        if x is not None:
            assert x.dtype == y.dtype and torch.equal(x, y), k
    assert a.total == b.total and a.hops == b.hops


@pytest.mark.parametrize("hops", ["otf", "dense"])
@pytest.mark.parametrize("name", ["sampler_cora_40_4.npz", "sampler_synthetic97_12_5.npz", "sampler_nba_5_4.npz"])
def test_device_built_sampler_philox_walks_match_host_built(name, hops):
    g = golden(name)
    n, L = int(g["n"]), int(g["L"])
    host = MerwSampler(n, g["u"], g["v"], g["p"], L, hops=hops)
    smp = MerwSampler(n, g["u"], g["v"], g["p"], L, hops=hops, build="device")
    same_tables(smp, host)
    for kw in (dict(epoch_begin=3, epoch_count=2, draw_source=DRAW_PHILOX), dict(node_begin=5, node_count=n - 9)):
        a, b = smp.sample(12, 99, **kw), host.sample(12, 99, **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    nodes = torch.from_numpy(np.random.default_rng(7).permutation(n)[: n // 3].astype(np.int32)).cuda()
    a, b = smp.sample(7, 5, epoch_begin=11, nodes=nodes), host.sample(7, 5, epoch_begin=11, nodes=nodes)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_device_tensor_rows_give_the_numpy_rows_tables():
    g = golden("sampler_citeseer_10_4.npz")
    n, L = int(g["n"]), int(g["L"])
    a = MerwSampler(n, g["u"], g["v"], g["p"], L, hops="otf", build="device")
    # int64 / float64 device tensors: converted on the device
    u, v, p = (torch.from_numpy(x).cuda() for x in (g["u"].astype(np.int64), g["v"].astype(np.int64), g["p"]))
    b = MerwSampler(n, u, v, p, L, hops="otf", build="device")
    same_tables(a, b)


def test_from_edge_file_passes_build(tmp_path):
    from oracle import merw
    g = golden("sampler_cornell_7_6.npz")
    f = str(tmp_path / "g.in")
    merw.write_edge_file(f, int(g["n"]), g["u"], g["v"], g["p"])
    a = MerwSampler.from_edge_file(f, int(g["L"]), build="device")
    b = MerwSampler.from_edge_file(f, int(g["L"]))
    assert a.host is None and b.host is not None
    same_tables(a, b)


def test_scale_er_2m_nodes_otf_tables_match_host():
    from tools.bench_sampler_large import er_graph
    n, u, v, p = er_graph(2_000_000, 16, 0)
    rng = np.random.default_rng(8)
    perm = rng.permutation(len(u))          # file order not sorted by source
    u, v, p = u[perm], v[perm], p[perm]
    host = MerwSampler(n, u, v, p, 6, hops="otf")
    smp = MerwSampler(n, u, v, p, 6, hops="otf", build="device")
    same_tables(smp, host)
