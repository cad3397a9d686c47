"""The exact-count scatter probes of tests/scatter_probe.py, proven without a GPU: for every case of its tables

  - the integer reference equals the fp64 CPU oracle (oracle/pagg_oracle.py, cell "sum" / "mean") EXACTLY, and the fp32
    oracle cast up exactly, on every tensor tests/test_gpu_scatter_exact.py compares;
  - every fp32 sum is exact in any order: per destination element the sum of |contribution| at the tensor's power-of-two
    scale stays below 2^24, so atomics, chunks, micro-batches and split-K must all return the reference's bits;
  - rows of X.grad that no path step and no masked node touch are +0 in the reference, one directly below and above every
    touched row;
  - the tables hit every edge class of det_scatter_kernel (pn_det.hip) -- the assertion lists what is left uncovered;
  - the comparison can fail: a dropped contribution of a crossing run, and one moved to the neighbouring row, are reported
    at the right row; and an integer model of the kernel's two passes, right on every sequence of the tables, is told from
    the plain sums under each of four faults by each of the three scatters' sequences."""
import numpy as np
import pytest
import torch

import dropout_probes as dp
import scatter_probe as sp


def test_tables_are_cut_for_the_kernels_chunk_size():
    assert sp.DET_CHUNK == sp.TABLES_CUT_FOR, "DET_CHUNK changed: revisit the run-length tables of tests/scatter_probe.py"


def _oracle(case, dtype):
    d = case.data
    G = d["G"].to(dtype)
    X = torch.zeros(d["N"], case.H)
    res = dp.oracle_run(case.variant, case.cell, sp.probe_params(case), X, d["sel"], d["ids"], d["codes"], case.W, case.L,
                        None, None, loss=lambda out, emb: (out * G).sum(), dtype=dtype)
    return res["grads"]


@pytest.mark.parametrize("cid", sp.CASE_IDS)
def test_integer_reference_is_the_oracle_and_order_independent(cid):
    case = sp.CASES[sp.CASE_IDS.index(cid)]
    want, bounds, touched = sp.reference(case)
    expected = {"X", "fc0.bias"} | {"%s%d.%s" % ("nei" if case.variant == "pagg" else "nets.", c, k)
                                    for c in range(sp.amp_len(case)) for k in ("weight", "bias")}
    if case.att is not None:
        expected |= {"attw.weight", "attw.bias"}
    assert set(want) == expected
    for dtype in (torch.float64, torch.float32):
        grads = _oracle(case, dtype)
        for name, w in want.items():
            assert grads[name].dtype == dtype
            assert torch.equal(grads[name].double(), w.double()), "%s: %s oracle differs: %s" % (
                name, dtype, sp.compare(case, {name: grads[name].double()}, {name: w.double()}))
    # order-independence, proven: every partial sum of every order is an integer below 2^24 times the tensor's scale
    for name, (scale, top) in bounds.items():
        assert top < 2 ** 24, "%s: sum of |numerators| %d at scale %g is not below 2^24" % (name, top, scale)
    # untouched rows are +0, and lie directly below and above touched ones
    x = want["X"]
    assert touched.any() and not x[torch.from_numpy(~touched)].view(torch.int32).any()
    assert (x[torch.from_numpy(touched)] != 0).all()
    t = np.flatnonzero(touched)
    assert t.min() >= 1 and t.max() <= case.data["N"] - 2 and not touched[t - 1].any() and not touched[t + 1].any()
    assert not sp.compare(case, want, want, touched)


def test_tables_hit_every_edge_class():
    have = {k: set() for k in ("row", "row-micro", "sel", "ego-homo", "ego-hetero", "case")}
    for case in sp.CASES:
        for k, v in sp.case_classes(case).items():
            have[k] |= v
    seq = set(sp.SEQUENCE_CLASSES)
    need = {
        "row": seq | set(sp.LANE_CLASSES),
        # chunks restart in every micro-batch: every crossing and boundary class again inside one
        "row-micro": set(sp.RUN_EDGES[1:]) | set(sp.K_SIZES[4:]),
        # DET_SEL and DET_EGO run the same kernel over S and S W keys: every class of the sequence itself can occur; the
        # lane-group classes would take more than a thousand masked nodes and are DET_ROW's
        "sel": seq, "ego-homo": seq, "ego-hetero": seq,
        "case": set(sp.PAIR_CLASSES),
    }
    missing = {k: sorted(v - have[k]) for k, v in need.items() if v - have[k]}
    assert not missing, "edge classes no case covers: %r" % (missing,)
    # what the GPU test's routes must each see: the three classes, both encoders, attention on and off, every H and L
    micro = [c for c in sp.CASES if c.data["micro"]]
    for cases in (sp.CASES, micro):
        assert {c.variant for c in cases} == {"homo", "hetero", "pagg"}
        assert {c.cell for c in cases} == {"sum", "mean"}
        assert {c.att is None for c in cases} == {True, False}
        assert {c.H for c in cases} == {32, 96, 128, 256, 288, 1024}
        assert {c.L for c in cases} == {1, 2, 4}
    for c in micro:
        sizes = [b - a for a, b in sp.micro_groups(c.data["S"], c.data["micro"])]
        assert len(sizes) >= 3 and sizes[-1] < sizes[0], (c.id, sizes)


def test_chunk_classes_on_hand_made_sequences():
    cc = sp.chunk_classes
    assert cc([7], 1, 32) == {"K = 1"}
    assert cc(np.arange(33), 33, 32) == {"K = chunk + 1", "all keys distinct", "chunk boundary that nothing crosses"}
    assert cc([5] * 64, 64, 32) == {"run filling exactly two aligned chunks"}         # (its head is at b = 0)
    got = cc([1] * 31 + [2] * 2 + [3] * 31, 64, 32)
    assert got == {"trail piece of one position", "lead piece of one position"}
    assert sp.lane_classes(1152, 32) == {sp.LANE_CLASSES[0]} and sp.lane_classes(1024, 32) == set()
    assert sp.lane_classes(384, 96) == {sp.LANE_CLASSES[1]} and sp.lane_classes(320, 96) == set()
    assert sp.lane_classes(40, 1024) == {sp.LANE_CLASSES[2]} and sp.lane_classes(32, 1024) == set()


def test_a_dropped_and_a_moved_contribution_are_reported_at_their_row():
    """the checker checked: mutate the reference on the CPU and compare it with the true one"""
    case = sp.CASES[sp.CASE_IDS.index("pagg-H96-12-chunks")]
    d = case.data
    want, _, touched = sp.reference(case)
    node, code = sp.po.plan(case.variant, d["ids"], d["codes"], d["S"], case.W, case.L)[:2]
    n = int(d["pool"][1])                       # run 1: sorted positions 50..99, crossing the chunk boundaries at 64 and 96
    q, t = (int(v[0]) for v in np.nonzero(node == n))
    dropped = sp.reference(case, drop=(q, t))[0]
    assert sp.differing_rows(dropped["X"], want["X"]) == [n]
    msgs = sp.compare(case, dropped, want, touched)
    x_msg = [m for m in msgs if m.startswith("X:")]
    assert len(x_msg) == 1 and "first at (row %d, column 0)" % n in x_msg[0] and "DET_ROW run [50, 100)" in x_msg[0]
    layer = "nei%d" % code[q, t]
    assert any(m.startswith(layer + ".bias") for m in msgs) and any(m.startswith("fc0.bias") for m in msgs)
    moved = sp.reference(case, move=(q, t))[0]
    assert sp.differing_rows(moved["X"], want["X"]) == [n, n + 1]
    msgs = sp.compare(case, moved, want, touched)
    assert any("first at (row %d, column 0)" % n in m for m in msgs)
    assert any("untouched row %d is not +0" % (n + 1) in m for m in msgs)
    assert not any(m.startswith(layer + ".bias") for m in msgs)        # the bank's column sums do not see a moved row


def test_the_run_length_tables_tell_a_wrong_two_pass_scatter_from_a_right_one():
    """det_scatter_kernel's passes restated in integers (scatter_probe.model_det_scatter): right, the model returns the
    plain sums on every key sequence of every case; with each of its faults -- all of the kind a norm-relative tolerance
    lets through -- at least one of the specified sequences returns other counts"""
    caught = {f: [] for f in sp.DET_FAULTS}
    for case in sp.CASES:
        d = case.data
        spans = [(0, d["S"])] + (sp.micro_groups(d["S"], d["micro"]) if d["micro"] else [])
        for g in spans:
            for which, keys in sp.scatter_keys(case.variant, d["sel"], d["ids"], d["codes"], case.W, case.L, g).items():
                if keys is None:
                    continue
                rows, vals = int(keys.max()) + 1, 1 + np.arange(len(keys)) % 7
                want = np.zeros(rows, np.int64)
                np.add.at(want, keys, vals)
                assert np.array_equal(sp.model_det_scatter(keys, vals, rows), want), (case.id, which, g)
                for f in sp.DET_FAULTS:
                    if not np.array_equal(sp.model_det_scatter(keys, vals, rows, fault=f), want):
                        caught[f].append((case.id, which))
    assert all(caught.values()), "faults no case's sequences show: %r" % [f for f, v in caught.items() if not v]
    for f, v in caught.items():         # each of the three scatters sees each fault
        assert {w for _, w in v} == {"row", "sel", "ego"}, (f, sorted({w for _, w in v}))
