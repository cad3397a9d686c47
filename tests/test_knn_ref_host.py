"""tests/knn_ref.py holds the GPU tests of pn_knn_search / pn_knn_vote to account; this file holds knn_ref.py to account, on
the CPU: the checker accepts the restatement's own answer on every case and rejects every named wrong implementation on at
least one, the integer cases are exact in fp32, the vote table's margins decide its labels, and what can be derived about
the work split without a device holds: pn_knn_plan and the workspace formula."""
import numpy as np
import pytest

import knn_ref as ref


def test_the_checker_accepts_the_reference_on_every_case():
    for i in range(len(ref.CASES)):
        Q, X, valid, exclude, k, metric, t = ref.case(i)
        want = ref.reference(Q, X, k, metric, valid, exclude)
        assert ref.check(want, Q, X, k, metric, valid, exclude, t) is None, ref.CASES[i]


def test_the_table_covers_the_edges():
    kinds, Sq, N, D, k, metric = (set(c[j] for c in ref.CASES) for j in range(6))
    assert Sq >= {1, 63, 64, 65, 130} and N >= {1, 127, 128, 129, 257, 400}
    assert D >= {1, 15, 16, 17, 33, 128} and k >= {1, 2, 5, 32, 64} and metric == {ref.COSINE, ref.DOT}
    assert kinds >= {"plain", "valid", "exclude", "self", "dead", "mix"}
    short = dead_q = dead_x = 0
    for i, c in enumerate(ref.CASES):
        t = ref.case(i)[6]
        live = t.cand.sum(axis=1)[t.qlive]
        short += int(((live < c[4]) & (live > 0)).sum())      # k > live candidates, with some
        dead_q, dead_x = dead_q + int(t.counts[0]), dead_x + int(t.counts[1])
    assert any(c[4] > c[2] for c in ref.CASES) and short > 0 and dead_q > 0 and dead_x > 0


@pytest.mark.parametrize("variant", ref.VARIANTS)
def test_the_checker_rejects_a_wrong_implementation(variant):
    said = []
    for i in range(len(ref.CASES)):
        Q, X, valid, exclude, k, metric, t = ref.case(i)
        msg = ref.check(ref.reference(Q, X, k, metric, valid, exclude, variant=variant), Q, X, k, metric, valid, exclude, t)
        if msg:
            said.append((ref.CASES[i], msg))
    assert said, variant


def test_the_checker_rejects_damaged_tails_counts_and_scores():
    Q, X, valid, exclude, k, metric, t = ref.case(2)
    for damage in ("tail", "count", "counts", "score", "dup"):
        got = ref.reference(Q, X, k, metric, valid, exclude)
        if damage == "tail":
            got.count[3] -= 1
        elif damage == "count":
            got.index[5, got.count[5] - 1], got.score[5, got.count[5] - 1] = -1, -np.inf
        elif damage == "counts":
            got.counts[1] += 1
        elif damage == "score":
            got.score[7, 0] += np.float32(4 * t.E[7].max() + 1e-6)
        else:
            got.index[9, 1] = got.index[9, 0]
        assert ref.check(got, Q, X, k, metric, valid, exclude, t) is not None, damage


def test_every_integer_case_is_exact_in_fp32():
    for i in range(len(ref.INT_CASES)):
        Q, X, k, index, score, mass = ref.int_case(i)
        assert mass < 2 ** 24, ref.INT_CASES[i]
        assert (Q == np.round(Q)).all() and (X == np.round(X)).all()
        got = ref.reference(Q, X, k, ref.DOT)       # and the float restatement agrees with the integer one, bit for bit
        assert (got.index == index).all() and (got.score[index >= 0] == score[index >= 0].astype(np.float32)).all()
    Sq, N, D, k, lo, hi = ref.INT_CASES[2]
    s = ref.int_case(2)[4]
    assert max((s[r] == s[r, 0]).sum() for r in range(Sq)) >= 4         # heavy ties


def test_the_vote_tables_margins_decide_the_labels():
    tie = voted = empty = 0
    for i in range(len(ref.VOTE_CASES)):
        index, score, count, bank_labels, C, T, labels, want = ref.vote_case(i)
        decided = want.margin > 1.0
        assert decided.all(), (ref.VOTE_CASES[i], np.flatnonzero(~decided), want.margin[~decided])
        if np.isinf(T):
            top = np.sort(want.prob, axis=1)[:, ::-1]
            tie += int(((top[:, 0] == top[:, 1]) & (want.label >= 0)).sum()) if C > 1 else 0
        assert np.allclose(want.prob.sum(axis=1)[want.label >= 0], 1.0)
        voted += int((want.label >= 0).sum())
        empty += int((want.label < 0).sum())
        assert want.confusion.sum() + want.skipped[0] == len(labels)
        assert (bank_labels < 0).any() and (bank_labels >= C).any() and (count == 0).any()
    assert tie > 0 and voted > 0 and empty > 0
    assert {c[3] for c in ref.VOTE_CASES} >= {1, 2, 7, 65}


def test_plan_fills_the_gpu_and_leaves_no_split_empty():
    splits, wgs, rt, ct = ref.plan(1299, 8192, 256, 20)
    assert (rt, ct) == (64, 128) and wgs >= 2 * 256 and wgs == -(-1299 // rt) * splits
    for Sq, N, asked in ((1299, 8192, 0), (1, 100, 0), (1, 1 << 20, 0), (2708, 2708, 0), (64, 400, 7), (64, 400, 3),
                         (5, 129, 1024), (8192, 8192, 0), (1 << 20, 300, 0)):
        splits, wgs, rt, ct = ref.plan(Sq, N, 16, 5, asked)
        tiles = -(-N // ct)
        assert 1 <= splits <= min(tiles, 1024) and (asked == 0 or splits == min(asked, tiles))
        bounds = [s * tiles // splits for s in range(splits + 1)]       # the kernel's share of split s
        assert bounds[0] == 0 and bounds[-1] == tiles and min(np.diff(bounds)) >= 1
        if asked == 0 and tiles * -(-Sq // rt) >= 512:
            assert wgs >= 512
    assert ref.plan(0, 100, 16, 5)[:2] == (0, 0) and ref.plan(100, 0, 16, 5)[:2] == (0, 0)


def test_the_workspace_is_linear():
    for Sq, N, D, k, splits in ((1299, 8192, 256, 20, 0), (1, 1, 1, 1, 1), (2708, 1000000, 256, 20, 0), (100, 400, 33, 64, 3),
                                (0, 50, 8, 2, 0), (50, 0, 8, 2, 0)):
        s = ref.plan(Sq, N, D, k, splits)[0]
        want = 64 + 8 * s * Sq * k + 4 * (Sq + N) * D + 4 * (Sq + N)
        assert ref.workspace_bytes(Sq, N, D, k, splits) == want + (-want) % 8
    # the 10 M-node configuration: a few GB, where the explicit matrix would be 400 TB
    assert ref.workspace_bytes(10_000_000, 10_000_000, 64, 20) < 16 * 2 ** 30


def test_refusals_need_no_device():
    from pathnet_amd import _lib
    import ctypes
    lib = _lib.load()
    need, out = ctypes.c_int64(-7), (ctypes.c_int64 * 4)(-7, -7, -7, -7)
    for Sq, N, D, k, splits in ((-1, 5, 4, 1, 0), (2 ** 31, 5, 4, 1, 0), (5, -1, 4, 1, 0), (5, 2 ** 31, 4, 1, 0), (5, 5, 0, 1, 0),
                                (5, 5, 8193, 1, 0), (5, 5, 4, 0, 0), (5, 5, 4, ref.MAX_K + 1, 0), (5, 5, 4, 1, -1),
                                (5, 5, 4, 1, 1025)):
        assert lib.pn_knn_workspace_bytes(Sq, N, D, k, splits, ctypes.byref(need)) == _lib.PN_ERR_ARG
        assert lib.pn_knn_plan(Sq, N, D, k, splits, out) == _lib.PN_ERR_ARG
        assert need.value == -7 and list(out) == [-7] * 4
    assert lib.pn_knn_workspace_bytes(5, 5, 4, 1, 0, None) == _lib.PN_ERR_ARG
    assert _lib.KNN_MAX_K == ref.MAX_K
