"""tests/sparse_fc0_ref.py on the CPU: the generators hold exactly the counts they claim, the inputs keep a one-entry mistake at
least 4 x above the derived bound in every value case, and the bound is not tighter than a correct fp32 sum (torch's dense fp32
product lies inside it).  Nothing here needs a GPU or the library."""
import numpy as np
import pytest
import torch

import sparse_fc0_ref as sr

IDS = ["%s-%s-H%d" % (name, N, H) for name, N, H in sr.VALUE_CASES]


def _counts(X):
    return (X != 0).sum(1), (X != 0).sum(0)


def test_row_staircase_holds_exactly_its_counts():
    X = sr.matrix("rows")
    rows, cols = _counts(X)
    assert X.shape == (200, 136) and rows.tolist() == sr.row_stair_counts()
    assert rows[:137].tolist() == list(range(137))
    # rows that end in a chunk of exactly 8 and 9 entries, rows of 63, 64 and 65, a full row
    assert {8, 9, 72, 73, 136, 63, 64, 65} <= set(rows.tolist()) and rows.max() == 136
    assert sorted(set(rows[137:].tolist())) == sorted(sr.ROW_STAIR_TAIL)
    assert cols.sum() == rows.sum()


def test_column_staircase_holds_exactly_its_counts():
    X = sr.matrix("cols")
    rows, cols = _counts(X)
    assert X.shape == (530, 72) and cols.tolist() == sr.col_stair_counts()
    assert cols[:28].tolist() == list(sr.COL_STAIR_HEAD) and cols[28:].max() < 64
    assert 530 % 64 == 18               # the bias blocks' last block: 18 rows, wavefronts 2 and 3 without one


def test_random_matrices_are_what_they_claim():
    X = sr.matrix("hidden")
    assert X.shape == (130, 40) and 0.35 < (X != 0).mean() < 0.45
    for N in sr.NODE_COUNTS:
        X = sr.matrix("nodes", N)
        assert X.shape == (N, 9) and X.any()
    X = sr.matrix("round")
    rows, cols = _counts(X)
    assert X.shape == (4100, 24) and 0.04 < (X != 0).mean() < 0.06
    assert (rows[4096:] >= 3).all() and cols.max() <= 520
    assert not sr.matrix("empty").any() and sr.matrix("empty").shape == (67, 13)
    X = sr.matrix("single")
    assert X.shape == (67, 13) and np.count_nonzero(X) == 1 and X[66, 12] == 0.75


def test_stored_values_and_operands_have_the_stated_magnitudes():
    for name, N, H in sr.VALUE_CASES:
        X, W, b, R = sr.operands(name, N, H)
        v = np.abs(X[X != 0])
        assert W.shape == (H, X.shape[1]) and b.shape == (H,) and R.shape == (X.shape[0], H)
        assert all(t.dtype == np.float32 for t in (X, W, b, R))
        assert (not len(v)) or (v.min() >= 0.5 and v.max() <= 1.5)
        assert np.abs(W).min() >= 0.25 and np.abs(W).max() <= 1.0 and (W < 0).any() and (W > 0).any()
        assert np.abs(R).min() >= 0.5 and np.abs(R).max() <= 1.5 and np.abs(b).max() <= 1.0


@pytest.mark.parametrize("N,F", [(1, 1), (2, 63), (4097, 5), (5, 4097), (256, 1023)])
def test_structure_matrices_are_about_30_percent_stored_with_empty_rows_and_columns(N, F):
    X = sr.structure_matrix(N, F)
    rows, cols = _counts(X)
    assert X.shape == (N, F) and X.dtype == np.float32
    if N * F == 1:
        assert X[0, 0] != 0
    if N * F >= 1000:
        assert 0.2 < (X != 0).mean() < 0.35
    assert N < 4 or (rows == 0).any()
    assert F < 4 or (cols == 0).any()


def test_carry_matrix_keeps_most_entries_behind_the_round_boundary():
    X = sr.carry_matrix()
    rows, _ = _counts(X)
    assert X.shape == (4097, 900) and rows[4096] == 900 and rows[:4096].sum() == 600


@pytest.mark.parametrize("name,N,H", sr.VALUE_CASES, ids=IDS)
def test_one_entry_mistakes_land_4x_above_the_bound(name, N, H):
    s = sr.sensitivity(*sr.operands(name, N, H))
    print({k: "%.3g" % v for k, v in s.items()})
    for k, v in s.items():
        assert v > 0.5 if k.startswith("share_") else v >= 4.0, (k, v)


@pytest.mark.parametrize("name,N,H", sr.VALUE_CASES, ids=IDS)
def test_torch_fp32_dense_product_lies_inside_the_bound(name, N, H):
    X, W, b, R = sr.operands(name, N, H)
    ref = sr.reference(X, W, b, R, relu=False)
    got = (torch.tensor(X) @ torch.tensor(W).T + torch.tensor(b)).numpy()
    worst = sr.ratio(got, ref["pre"], ref["bound_Xh"]).max()
    got_w = (torch.tensor(R).T @ torch.tensor(X)).numpy()
    worst_w = sr.ratio(got_w, ref["g_w"], ref["bound_g_w"]).max()
    got_b = torch.tensor(R).sum(0).numpy()
    worst_b = sr.ratio(got_b, ref["g_b"], ref["bound_g_b"]).max()
    print("torch fp32 error / bound: Xh %.3f  g_w %.3f  g_b %.3f" % (worst, worst_w, worst_b))
    assert worst <= 1.0 and worst_w <= 1.0 and worst_b <= 1.0


def test_reference_and_ratio_on_a_case_worked_by_hand():
    X = np.array([[0.5, 0.0, -1.0], [0.0, 0.0, 0.0]], np.float32)
    W = np.array([[1.0, 0.5, 0.25], [-0.5, 1.0, -1.0]], np.float32)
    b = np.array([0.5, -1.0], np.float32)
    R = np.array([[1.0, -0.5], [0.5, 1.5]], np.float32)
    ref = sr.reference(X, W, b, R, relu=True)
    assert ref["pre"].tolist() == [[0.75, -0.25], [0.5, -1.0]] and ref["Xh"].tolist() == [[0.75, 0.0], [0.5, 0.0]]
    assert ref["g_w"].tolist() == [[0.5, 0.0, -1.0], [-0.25, 0.0, 0.5]] and ref["g_b"].tolist() == [1.5, 1.0]
    assert ref["bound_Xh"].tolist() == [[6 * sr.U32 * 1.25, 6 * sr.U32 * 2.25], [4 * sr.U32 * 0.5, 4 * sr.U32 * 1.0]]
    assert ref["bound_g_w"].tolist() == [[5 * sr.U32 * 0.5, 0.0, 5 * sr.U32 * 1.0], [5 * sr.U32 * 0.25, 0.0, 5 * sr.U32 * 0.5]]
    assert ref["bound_g_b"].tolist() == [6 * sr.U32 * 1.5, 6 * sr.U32 * 2.0]
    gated = sr.reference(X, W, b, R, relu=True, gate=ref["Xh"] > 0)
    assert gated["g_w"].tolist() == [[0.5, 0.0, -1.0], [0.0, 0.0, 0.0]] and gated["g_b"].tolist() == [1.5, 0.0]
    r = sr.ratio(np.array([1.0, 0.0, 2.0]), np.array([1.0, 0.0, 1.0]), np.array([0.0, 0.0, 0.5]))
    assert r.tolist() == [0.0, 0.0, 2.0]
    assert sr.ratio(np.array([1.0]), np.array([0.0]), np.array([0.0])).tolist() == [np.inf]
