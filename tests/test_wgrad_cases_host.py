"""The tables of tests/wgrad_cases.py, proven without a GPU:

  - the constants the restatement uses are the ones the sources define (a changed K tile, output tile or CU count must
    send someone back to the case table);
  - every edge class is contained in at least one row that carries one-group probes, for each of wgradh_kernel,
    wgrad4_kernel and wgrad3_kernel -- the assertion lists what is left uncovered;
  - the restated loops agree with a literal walk of the kernels' index arithmetic: every K tile is taken by exactly one
    split, every split of the reduce by exactly one lane group;
  - the probes name the groups they claim to: a one-group gradient leaves every other row of dG exactly zero in the oracle;
  - on the localized probe rows the fp32 oracle, held to the fp64 oracle, passes the very assertion the GPU test makes of
    the kernels (tests/wgrad_cases.check), with no tensor vacuous: the bound is reachable in fp32 and the probes carry signal."""
import pytest
import torch

import wgrad_cases as wc


def test_restated_constants_are_the_sources():
    assert wc.PARSED == wc.RESTATED
    assert (wc.KT["wgradh"], wc.KT["wgrad4"], wc.KT["wgrad3"], wc.PARSED["PN_WGRAD_CUS_SHARED"]) == wc.TABLES_CUT_FOR, \
        "a K tile or the CU count changed: revisit the case table of tests/wgrad_cases.py"


def test_every_edge_class_is_in_the_table_for_every_kernel():
    cov = wc.coverage()
    assert set(cov) == set(wc.KERNELS)
    for k in wc.KERNELS:
        assert set(cov[k]) == set(wc.APPLICABLE[k]) and set(wc.APPLICABLE[k]) <= set(wc.ALL_CLASSES)
    # every class of the list is asked of at least one kernel, and of wgrad3 all of them
    assert set(wc.APPLICABLE["wgrad3"]) == set(wc.ALL_CLASSES)
    missing = {k: sorted(cl for cl, rows in cov[k].items() if not rows) for k in wc.KERNELS}
    assert not any(missing.values()), "edge classes no table row contains: %r" % (missing,)


def test_table_stays_small():
    for c in wc.CASES:
        assert c.S <= wc.N <= 400 and wc.F <= 48
        assert max(wc.rows_of(c, b) for b in range(len(wc.micro_batches(c)))) <= 224 * 128 + c.W * c.L
    assert len(wc.CASES) <= 48
    assert {(c.variant, wc.cell_of(c)) for c in wc.CASES} >= {("homo", "lstm"), ("homo", "gru"), ("homo", "rnn"), ("pagg", "rnn"),
                                                               ("hetero", "lstm")}
    assert {c.L for c in wc.CASES} == {1, 3, 4, 6}


@pytest.mark.parametrize("kt", [16, 32])
def test_strided_tiles_partition_the_rows(kt):
    """a literal walk of the kernels' loops: split z, trip i -> tile z + i nsplit, rows clamped and masked"""
    for c in wc.CASES:
        nz = wc.split_of(c)
        for b in range(len(wc.micro_batches(c))):
            R = wc.rows_of(c, b)
            ns = wc.launched(R, nz, kt)
            assert 1 <= ns <= nz
            seen = [0] * R
            for z in range(ns):
                mine = wc.my_tiles(z, R, ns, kt)
                assert mine >= 1
                trips = mine + (mine & 1 if kt == 16 else 0)        # wgradh / wgrad4: two tiles per trip
                for i in range(trips):
                    row0 = (z + min(i, mine - 1) * ns) * kt
                    for r in range(row0, row0 + kt):
                        if i < mine and r < R:
                            seen[r] += 1
            assert seen == [1] * R, (wc.case_id(c), b)


def test_reduce_loops_take_every_split_once():
    for n in range(1, 257):
        loops = wc.reduce_loops(n)
        g, u = wc.PARSED["REDUCE_GROUPS"], wc.PARSED["REDUCE_UNROLL"]
        taken = []
        for zg, (rounds, tail) in enumerate(loops):
            z = zg
            for _ in range(rounds):
                taken += [z + g * k for k in range(u)]
                z += g * u
            for _ in range(tail):
                taken.append(z)
                z += g
        assert sorted(taken) == list(range(n)), n
    # the counts the table is asked to contain are the ones at which a lane group changes loops
    shapes = {n: tuple(wc.reduce_loops(n)) for n in wc.REDUCE_NSPLIT}
    assert len(set(shapes.values())) == len(shapes)
    assert shapes[28] == ((0, 7),) * 4 and shapes[29] == ((1, 0), (0, 7), (0, 7), (0, 7)) and shapes[32] == ((1, 0),) * 4
    assert shapes[33] == ((1, 1), (1, 0), (1, 0), (1, 0)) and shapes[61] == ((2, 0), (1, 7), (1, 7), (1, 7))


def test_split_arithmetic_at_known_shapes():
    # the headline shape (Cora: 140 masked nodes, W = 40, L = 4, H = 128 LSTM): 112 splits of 200 K tiles of 16 rows
    assert wc.tiles(128, 4) == 2 and wc.wgrad_split(140 * 40, 4, 128, 4) == 112
    assert [wc.tiles(H, G) for H, G in ((32, 4), (32, 1), (64, 4), (128, 1), (96, 4), (160, 4), (256, 4), (288, 4))] == [1, 1, 1, 1, 2, 6, 8, 15]
    assert wc.cus(4.5e5, 128, 4) == 224 and wc.cus(4.7e5, 128, 4) == 256          # the branch this table leaves alone
    assert max(wc.cus(wc.rows_of(c, 0), c.H, wc.gates(c)) for c in wc.CASES) == 224


def test_probes_are_localized():
    """under a one-group gradient only that group's W L rows reach the recurrence: the gradient of the loss with respect to
    the recurrent input y [P, L, H] -- one row per reduction row r = q L + t -- is exactly zero outside the rows
    (s - g0) W L .. + W L of group s, and not zero inside (homo / PAGG: slot q belongs to group q // W)"""
    from oracle import pagg_oracle as po
    for c in (wc.CASES[0], wc.CASES[23]):
        assert c.variant != "hetero"
        d, params = wc.make_inputs(c), wc.make_params(c)
        leaf = {k: v.clone().requires_grad_(True) for k, v in params.items()}
        out, mid = po.forward(c.variant, leaf, d["X"], d["ids"], d["codes"], d["sel"], c.W, c.L, drop_seq=d["mask_seq"],
                              drop_cls=d["mask_cls"], dtype=torch.float64, return_intermediates=True, cell=c.cell)
        wl = c.W * c.L
        for kind, s in wc.probes(c)[1:]:
            g = wc.upstream(c, d["G"], s)
            assert g[s].abs().max() > 0 and not g[:s].any() and not g[s + 1:].any()
            dy = torch.autograd.grad(out, mid["y"], g.double(), retain_graph=True)[0].reshape(c.S * wl, c.H)
            assert not dy[:s * wl].any() and not dy[(s + 1) * wl:].any(), (wc.case_id(c), kind)
            assert (dy[s * wl:(s + 1) * wl].abs().amax(dim=1) > 0).all(), (wc.case_id(c), kind)
    # the straddling group holds the last row of the last whole K tile and the first row of the ragged one
    for c in wc.CASES:
        for b in range(len(wc.micro_batches(c))):
            for kt in (16, 32):
                s = wc.straddling_group(c, b, kt)
                if s is not None:
                    g0, wl, edge = wc.micro_batches(c)[b][0], c.W * c.L, wc.rows_of(c, b) // kt * kt
                    assert (s - g0) * wl < edge < (s - g0 + 1) * wl


HOST_PROBES = [(0, "dense"), (0, "first"), (0, "last"), (1, "dense"), (1, "first"), (1, "last"), (2, "dense"), (2, "first"),
               (2, "last"), (3, "dense"), (3, "last")]


@pytest.mark.parametrize("row,kind", HOST_PROBES)
def test_fp32_oracle_passes_the_gpu_tests_assertion(row, kind):
    c = wc.HOST_ROWS[row]
    full = [k for k, _ in wc.probes(c) if kind in k.split("+")]
    assert len(full) == 1
    group = dict(wc.probes(c))[full[0]]
    assert group == {"dense": None, "first": 0, "last": c.S - 1}[kind]
    want = wc.oracle_grads(c, torch.float64, which=full)[full[0]]
    out, grads = wc.oracle_grads(c, torch.float32, which=full)[full[0]]
    msgs = wc.check(c, full[0], group, out, grads, want, "oracle32")
    assert not msgs, msgs
    # the probe carries signal in every recurrent tensor: the smallest |g|_inf is far above the noise floor
    assert min(float(want[1][k].abs().max()) for k in wc.recurrent_names(c)) > 1e-3
