"""The tables of tests/rgrad_cases.py, proven without a GPU:

  - the constants the restatement uses are the ones the sources define (a changed tile, split rule or dispatch floor must
    send someone back to the case table);
  - every edge class is contained in at least one row that carries one-group probes, for the GATE and the no-GATE
    instantiation of rgrad_kernel -- the assertion lists what is left uncovered;
  - the restated loops agree with a literal walk of the kernel's index arithmetic: every reduction row is taken by exactly
    one split, in a real (not a zero or clamped) tile;
  - the restated route() agrees with the library where the library shows it without a GPU: the xpad slot of
    pn_pagg_workspace_bytes appears between N = 2047 and N = 2048 exactly where route() says "rgrad+xpad";
  - the probes are what they claim: the pinned groups visit every edge node, and under a one-group gradient the rows of
    dXh and dZ outside the visited nodes are exactly zero in the oracle;
  - conditions on the reference: on HOST_ROWS (at least one row per route) the fp32 oracle, held to the fp64 oracle, passes
    the very assertion the GPU test makes (tests/rgrad_cases.check).  Its largest share of the bound over the node-level
    tensors is printed; measured: 0.027 of the bound at the most (homo, N = 513, the "first" probe), 0.005 .. 0.02 elsewhere --
    fp32 rounding over a few thousand rows, far from the bound, which therefore measures the kernel;
  - sensitivity: from the fp64 oracle's own dXh, dZ, Xh and X a NumPy reduction reproduces the oracle's gradients, and with
    ONE edge row dropped, doubled or replaced by its clamped neighbour it fails check() -- for every probe of HOST_ROWS and
    every edge node of the probe."""
import functools

import numpy as np
import pytest
import torch

import rgrad_cases as rc
from oracle import pagg_oracle as po


def test_restated_constants_are_the_sources():
    assert rc.PARSED == rc.RESTATED
    p = rc.PARSED
    assert (p["R_BM"], p["R_BN"], p["R_KT"], p["SPLIT_WORKGROUPS"], p["SPLIT_MIN_TILES"], p["PAYS_ROWS"], p["XPAD_MIN_NODES"],
            p["XPAD_CAP_BYTES"]) == rc.TABLES_CUT_FOR, "a constant of pn_rgrad.hip / xpad_floats changed: revisit the case table of tests/rgrad_cases.py"


def test_every_edge_class_is_in_the_table_for_every_instantiation():
    cov, once = rc.coverage()
    assert set(cov) == set(rc.INSTANTIATIONS)
    for k in rc.INSTANTIATIONS:
        assert set(cov[k]) == set(rc.APPLICABLE[k]) and set(rc.APPLICABLE[k]) <= set(rc.ALL_CLASSES)
    assert set(rc.APPLICABLE["gate"]) | set(rc.APPLICABLE["nogate"]) | set(rc.ONCE) == set(rc.ALL_CLASSES)
    missing = {k: sorted(cl for cl, rows in cov[k].items() if not rows) for k in rc.INSTANTIATIONS}
    missing["once"] = sorted(cl for cl, rows in once.items() if not rows)
    assert not any(missing.values()), "edge classes no table row contains: %r" % (missing,)


def test_table_rows_and_their_routes():
    """the rows are about the kernel: every row but the one below the dispatch floor runs both GEMMs on it"""
    for c in rc.CASES:
        rt = rc.route_of(c)
        if c.N == 2047:
            assert c.knob == rc.KNOB_DEFAULT and rt == {"g_bank_w": "gemm", "g_fc0_w": "gemm"}
            continue
        assert rt["g_bank_w"] == "rgrad" and rt["g_fc0_w"] == ("rgrad" if c.F % 4 == 0 else "rgrad+xpad"), rc.case_id(c)
        assert c.knob == (rc.KNOB_ALWAYS if c.N < 2048 else rc.KNOB_DEFAULT)
        assert c.S <= c.N and c.H % 32 == 0
    assert len(rc.CASES) <= 40
    assert {rc.route_of(c)["g_fc0_w"] for c in rc.HOST_ROWS} == {"rgrad", "rgrad+xpad", "gemm"}
    assert {rc.instantiation(c) for c in rc.HOST_ROWS} == set(rc.INSTANTIATIONS)
    for c in rc.CASES:
        print("%-52s bank %-6s nz %2d   fc0 %-10s nz %2d" % (rc.case_id(c), rc.route_of(c)["g_bank_w"], rc.nz_of(c, "g_bank_w"),
                                                         rc.route_of(c)["g_fc0_w"], rc.nz_of(c, "g_fc0_w")))


def test_split_arithmetic_at_known_shapes():
    # Cora (N = 2708, F = 1433 -> 1436, H = 128, L = 4): ten splits of 85 K tiles for both GEMMs
    assert rc.out_tiles(512, 128) == 4 and rc.out_tiles(128, 1433) == 12 and rc.nz(2708, 512, 128) == 10 and rc.nz(2708, 128, 1433) == 10
    assert [rc.nz(R, 128, 128) for R in (20, 32, 33, 255, 257, 511, 512, 513, 545, 767, 768, 773)] == [1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3]
    assert rc.nz(6001, 1536, 256) == 22 and rc.nz(6001, 256, 8) == 23 and rc.nz(8500, 1024, 256) == 32 and rc.nz(10 ** 7, 128, 128) == 512
    assert [rc.ragged_owner(R, rc.nz(R, 128, 128)) for R in (512, 513, 545, 773)] == [None, 0, 1, 0]
    assert [rc.my_tiles(z, 513, 2) for z in range(2)] == [9, 8] and [rc.my_tiles(z, 773, 3) for z in range(3)] == [9, 8, 8]


def test_strided_tiles_partition_the_rows():
    """a literal walk of rgrad_kernel's loop: split z, trip i -> tile z + min(i, my_tiles - 1) nz, two tiles per trip, rows
    clamped to R - 1 and masked by i < my_tiles && row < R"""
    for c in rc.CASES:
        for g in rc.GEMMS:
            R, n = c.N, rc.nz_of(c, g)
            seen = [0] * R
            for z in range(n):
                mine = rc.my_tiles(z, R, n)
                assert mine >= 1
                for i in range(mine + (mine & 1)):
                    row0 = (z + min(i, mine - 1) * n) * rc.KT
                    for r in range(row0, row0 + rc.KT):
                        assert min(r, R - 1) < R
                        if i < mine and r < R:
                            seen[r] += 1
            assert seen == [1] * R, (rc.case_id(c), g)


def _lib_bytes(variant, N, F, H, L, deterministic=False):
    from pathnet_amd import _lib, modules
    return modules.workspace_bytes(variant, N, F, H, rc.C, 12, 4, L, deterministic=deterministic, compact=_lib.COMPACT_OFF)


def test_route_agrees_with_the_workspace_layout():
    """the xpad slot is the one trace of the route that the library shows without a GPU: N F4 floats that appear at N = 2048"""
    cap = rc.PARSED["XPAD_CAP_BYTES"]
    # (F, deterministic): F % 4 != 0 small and at Cora's width, exactly at the cap (2048 x 32768 x 4 = 256 MB) and one quad past
    # it, F % 4 == 0, the deterministic shape
    shapes = [(5, False), (127, False), (129, False), (1433, False), (32765, False), (32769, False), (40001, False),
              (4, False), (128, False), (132, False), (129, True), (1433, True)]
    for variant, L in (("homo", 3), ("pagg", 4)):
        for F, det in shapes:
            F4 = -(-F // 4) * 4
            Ns = (2046, 2047, 2048, 2049)
            b = [_lib_bytes(variant, N, F, 32, L, det) for N in Ns]
            # without the slot the restated rule gives each N, the layout grows by the same bytes per node on either side of the
            # floor (64 slots, each rounded up to 256 bytes: the slack) -- at the cap the slot is there at 2 048 and gone at 2 049
            rest = [x - 4 * rc.xpad_floats(N, F, det) for x, N in zip(b, Ns)]
            below = rest[1] - rest[0]
            assert abs(rest[2] - rest[1] - below) <= 64 * 256 and abs(rest[3] - rest[2] - below) <= 64 * 256, (variant, F, det, b)
            # ... and the raw byte counts step by the whole copy or not at all
            at = b[2] - b[1] - (b[1] - b[0])
            stepped = at >= 2048 * F4 * 4 - 64 * 256
            assert stepped or at <= 64 * 256, (variant, F, det, b)
            want = rc.route(variant, 2048, F, 32, L, rc.KNOB_DEFAULT, det)["g_fc0_w"]
            assert stepped == (want == "rgrad+xpad"), (variant, F, det, want, below, at)
            assert (rc.xpad_floats(2048, F, det) > 0) == stepped
            assert rc.route(variant, 2047, F, 32, L, rc.KNOB_DEFAULT, det)["g_fc0_w"] == ("det" if det else "gemm")
            # the knob forces the kernel below the floor, never the copy
            assert rc.route(variant, 2047, F, 32, L, rc.KNOB_ALWAYS, det)["g_fc0_w"] == ("det" if det else "rgrad" if F % 4 == 0 else "gemm")
    assert rc.xpad_floats(2048, 32765, False) * 4 == cap and rc.xpad_floats(2048, 32769, False) == 0
    # the slot, once there, grows with N by F4 floats a node
    assert _lib_bytes("homo", 2049, 129, 32, 3) - _lib_bytes("homo", 2048, 129, 32, 3) >= 132 * 4
    assert rc.route("homo", 4096, 8, 100, 3) == {"g_bank_w": "rgrad", "g_fc0_w": "rgrad"}          # H is padded to 128
    assert rc.route("homo", 4096, 8, 32, 3, knob=0) == {"g_bank_w": "gemm", "g_fc0_w": "gemm"}
    assert rc.route("homo", 20000, 8, 32, 3, compact=2047)["g_bank_w"] == "gemm" and rc.route("homo", 20000, 8, 32, 3, compact=2048)["g_bank_w"] == "rgrad"


def test_probe_groups_visit_the_edges():
    for c in rc.CASES:
        if c.variant == "hetero":
            assert rc.probes(c) == [("dense", None)]
            continue
        d, edges, R = rc.make_inputs(c), rc.edge_nodes(c), c.N
        want = {0, R - 1, min(31, R - 1), min(32, R - 1)} | ({R // rc.KT * rc.KT} if R % rc.KT else set())
        assert want <= set(edges) and edges[0] == 0 and edges[-1] == R - 1
        for g in rc.GEMMS:              # one node in a tile owned by each split z, for the splits of either GEMM
            assert all(rc.split_nodes(c, g).values()), (rc.case_id(c), g)
        assert d["sel"][0] == 0 and d["sel"][-1] == R - 1 and len(set(d["sel"].tolist())) == c.S
        for kind, s in rc.probes(c)[1:]:
            assert set(d["ids"][s].reshape(-1).tolist()) == set(edges), (rc.case_id(c), kind)
            used = set(d["codes"][s].reshape(-1).tolist())
            assert {0, c.L - 1} <= used and used == (set(range(c.L)) if kind == "first" else {0, c.L - 1}), (rc.case_id(c), kind)


# ---- the oracles of HOST_ROWS ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _host(row):
    c = rc.HOST_ROWS[row]
    d = rc.make_inputs(c)
    want, inner, mid = rc.oracle_grads(c, torch.float64, inputs=d, return_intermediates=True)
    got32 = rc.oracle_grads(c, torch.float32, inputs=d)
    return c, d, want, inner, mid, got32


def _operands(c, d, mid, dXh, dy):
    """the kernel's operands out of the fp64 oracle: dZ' [N, L, H] (the scatter of dy over (node, code), gated), Xh [N, H],
    dXh' [N, H] (gated), X [N, F]"""
    node, code = po.plan(c.variant, d["ids"], d["codes"], c.S, c.W, c.L)[:2]
    Xh, y = mid["Xh"].numpy(), mid["y"].numpy().reshape(-1, c.H)
    dy, dXh = dy.numpy().reshape(-1, c.H).copy(), dXh.numpy().copy()
    if c.variant == "homo":         # (y = relu(Z): y > 0 where Z > 0; Xh = relu(fc0): likewise)
        dy *= y > 0
        dXh *= Xh > 0
    dZ = np.zeros((c.N, c.L, c.H))
    np.add.at(dZ, (node.reshape(-1), code.reshape(-1)), dy)
    return dZ, Xh, dXh, d["X"].double().numpy()


def _reduce(c, ops, weight=None):
    """{name: gradient} of the node-level tensors as plain sums over the rows of the graph, row n weighted by weight[n]"""
    dZ, Xh, dXh, X = ops
    w = np.ones(c.N) if weight is None else weight
    out = {"fc0.weight": np.einsum("n,nh,nf->hf", w, dXh, X), "fc0.bias": np.einsum("n,nh->h", w, dXh)}
    for code, b in enumerate(rc.bank_names(c)):
        out[b + ".weight"] = np.einsum("n,ni,nj->ij", w, dZ[:, code], Xh)
        out[b + ".bias"] = np.einsum("n,ni->i", w, dZ[:, code])
    return out


def _row_term(c, ops, n):
    """row n's own term of every sum of _reduce"""
    dZ, Xh, dXh, X = ops
    out = {"fc0.weight": np.outer(dXh[n], X[n]), "fc0.bias": dXh[n].copy()}
    for code, b in enumerate(rc.bank_names(c)):
        out[b + ".weight"] = np.outer(dZ[n, code], Xh[n])
        out[b + ".bias"] = dZ[n, code].copy()
    return out


HOST_PROBES = [(r, k) for r in range(len(rc.HOST_ROWS)) for k in ("dense", "first", "last")]


@pytest.mark.parametrize("row,kind", HOST_PROBES)
def test_probes_are_localized_and_the_reduction_is_the_oracles(row, kind):
    c, d, want, inner, mid, _ = _host(row)
    ops = _operands(c, d, mid, *inner[kind])
    dZ, Xh, dXh, X = ops
    mine = _reduce(c, ops)
    for k in rc.node_level_names(c):
        ref = want[kind][1][k].numpy()
        assert np.abs(mine[k] - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (rc.case_id(c), kind, k)
    if kind == "dense":
        return
    # under a one-group gradient the rows of dXh / dZ outside the group's nodes are exactly zero, and every visited node
    # has a row of both; a distance layer the probe's codes leave out has an exactly zero reference
    edges = np.asarray(rc.edge_nodes(c))
    other = np.setdiff1d(np.arange(c.N), edges)
    assert not dZ[other].any() and not dXh[other].any()
    assert (np.abs(dZ[edges]).max(axis=(1, 2)) > 0).all() and (np.abs(dXh[edges]).max(axis=1) > 0).all()
    if kind == "last":
        for code in range(1, c.L - 1):
            b = rc.bank_names(c)[code]
            assert not want[kind][1][b + ".weight"].any() and not want[kind][1][b + ".bias"].any()


SHARES = []


@pytest.mark.parametrize("row,kind", HOST_PROBES)
def test_fp32_oracle_passes_the_gpu_tests_assertion(row, kind):
    c, d, want, inner, mid, got32 = _host(row)
    group = dict(rc.probes(c))[kind]
    out, grads = got32[kind]
    shares = []
    msgs = rc.check(c, kind, group, out, grads, want[kind], "oracle32", shares)
    assert not msgs, msgs
    SHARES.append(max(shares))
    print("oracle32 %s %s: largest share of the bound over the node-level tensors %.3g (so far, all rows: %.3g)"
          % (rc.case_id(c), kind, max(shares), max(SHARES)))
    # the fp32 oracle must sit well inside the bound, or the bound says nothing about the kernel
    assert max(shares) < 0.25
    # the probe carries signal in the tensors it is about
    names = [k for k in rc.node_level_names(c) if want[kind][1][k].any()]
    assert "fc0.weight" in names and len(names) >= 4
    assert min(float(want[kind][1][k].abs().max()) for k in names) > 1e-4


@pytest.mark.parametrize("row,kind", [(r, k) for r, k in HOST_PROBES if k != "dense"])
def test_one_wrong_edge_row_fails_the_assertion(row, kind):
    """a dropped row, a doubled row, a row replaced by its clamped neighbour (the next edge node; for the last row the one
    before: what a load clamped to the wrong row would bring)"""
    from gradcheck import grad_report
    c, d, want, inner, mid, _ = _host(row)
    group = dict(rc.probes(c))[kind]
    ops = _operands(c, d, mid, *inner[kind])
    base, edges = _reduce(c, ops), rc.edge_nodes(c)
    names = rc.node_level_names(c)
    ref = {k: want[kind][1][k] for k in names}
    worst = {}
    for i, e in enumerate(edges):
        nb = edges[i + 1] if i + 1 < len(edges) else edges[i - 1]
        mine, theirs = _row_term(c, ops, e), _row_term(c, ops, nb)
        for what, delta in (("dropped", {k: -mine[k] for k in names}), ("doubled", mine),
                            ("clamped", {k: theirs[k] - mine[k] for k in names})):
            grads = dict(want[kind][1])
            grads.update({k: torch.from_numpy(base[k] + delta[k]) for k in names})
            msgs = rc.check(c, kind, group, want[kind][0], grads, want[kind], "%s row %d" % (what, e))
            assert msgs, "%s %s: row %d %s goes unnoticed" % (rc.case_id(c), kind, e, what)
            rows, _ = grad_report({k: grads[k] for k in names}, ref)
            excess = max(err / tol for err, tol, _ in rows.values())
            worst[what] = min(worst.get(what, float("inf")), excess)
    assert min(worst.values()) > 1.0, worst
    print("sensitivity %s %s: %d edge rows; each fails check() when dropped / doubled / clamped, by at least %s times the bound"
          % (rc.case_id(c), kind, len(edges), ", ".join("%.3g" % worst[w] for w in ("dropped", "doubled", "clamped"))))
