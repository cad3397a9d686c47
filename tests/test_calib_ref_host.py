"""The NumPy restatement tests/calib_ref.py against itself and against torch, on the CPU: the fp64 definition stays inside the
derived bounds of the long-double yardstick, and every case the GPU tests hold pn_calib_sweep to is decidable."""
import math

import numpy as np
import pytest
import torch

import calib_ref as ref
import ensemble_ref as eref


@pytest.mark.parametrize("kind", ref.SWEEP_KINDS)
def test_sweep_fp64_inside_the_bounds_and_every_gpu_case_decidable(kind):
    worst = np.inf
    for case in ref.sweep_cases(kind):
        C, S, R, T = case
        x, y, temps = ref.sweep_inputs(kind, case)
        lo, hi = ref.sweep(x, y, temps), ref.sweep(x, y, temps, np.longdouble)
        assert (lo.counts == hi.counts).all() and lo.counts.sum() == S, case
        tol_rows = ref.tol_row_nll(hi.q, C, R)
        same_inf = np.isinf(lo.row_nll) & (lo.row_nll == hi.row_nll)
        err = np.where(same_inf, 0, np.abs(lo.row_nll - hi.row_nll)).astype(np.float64)
        assert (err <= tol_rows).all(), (case, float((err / tol_rows).max()))
        fin = np.isfinite(hi.nll.astype(np.float64))
        assert (np.isfinite(lo.nll) == fin).all(), case
        e_nll = np.abs(lo.nll[fin] - hi.nll[fin]).astype(np.float64)
        assert (e_nll <= ref.tol_nll(hi.row_nll.astype(np.float64), tol_rows)[fin]).all(), case
        ok, ratio = ref.decidable(lo, hi, C, R)
        assert ok, "%s %s: the gap is %g x the bound" % (kind, case, ratio)
        worst = min(worst, ratio)
        assert lo.best == hi.best and lo.tau == hi.tau, case
        if S == 0:
            assert lo.best == -1 and lo.tau == 1.0
        if kind == "badgrid" and S:
            assert np.isinf(lo.nll[0]) and lo.best % 4 != 0
    print("%s: the smallest gap is %.3g x the bound" % (kind, worst))


def test_issue_family_is_decidable_on_the_default_grid():
    """the family of the issue over its own (C, S, R) lattice, at the sizes the long-double restatement affords"""
    for C in (2, 7, 17, 65, 1025):
        for S in (1, 5, 64, 65, 1000):
            for R in (1, 2, 5):
                if S * C * R > 70_000:
                    continue
                for true in ref.TRUE_TEMPS:
                    x, y = ref.make_case(C, S, R, true, seed=C + S + R)
                    lo, hi = ref.sweep(x, y, ref.DEFAULT_GRID), ref.sweep(x, y, ref.DEFAULT_GRID, np.longdouble)
                    ok, ratio = ref.decidable(lo, hi, C, R)
                    assert ok and lo.best == hi.best, (C, S, R, true, ratio)


def test_single_sample_row_nll_is_cross_entropy():
    for C, S in ((7, 65), (130, 9)):
        x, y = ref.make_case(C, S, 1, 1.0, seed=3)
        got = ref.sweep(x, y, ref.DEFAULT_GRID)
        xt, yt = torch.from_numpy(x[0]).double(), torch.from_numpy(y)
        for t, tau in enumerate(ref.DEFAULT_GRID):
            want = torch.nn.functional.cross_entropy(xt / tau, yt, reduction="none").numpy()
            tol = 2 * ref.tol_row_nll(got.q[:, t], C, 1) + 4 * ref.U * np.abs(want)
            assert (np.abs(got.row_nll[:, t] - want) <= tol).all(), (C, S, tau)


def test_column_sum_order_is_the_documented_one():
    rng = np.random.default_rng(0)
    for S in (0, 1, 255, 256, 257, 700):
        r = rng.random((S, 3))
        want = np.zeros(3)
        for p in range(0, S, ref.PART):
            part = np.zeros(3)
            for s in range(p, min(p + ref.PART, S)):
                part += r[s]
            want += part
        assert (ref.column_sums(r) == want).all()


def test_scaled_add_restatement():
    C, S, R = 9, 40, 3
    x = eref.make_logits("nonfinite", R, S, C, seed=2)
    a, b = eref.new_state(S, C), eref.new_state(S, C)
    eref.add(a, x)
    assert ref.add_scaled(b, x, 1.0) == 0
    for f in a._fields:
        assert (getattr(a, f) == getattr(b, f)).all(), f          # tau == 1: the plain add, bit for bit
    for tau in (0.37, 2.5):
        lo, hi = eref.new_state(S, C), eref.new_state(S, C, np.longdouble)
        ref.add_scaled(lo, x, tau)
        ref.add_scaled(hi, x, tau)
        assert (lo.votes == a.votes).all() and (lo.count == a.count).all() and (lo.bad == a.bad).all()
        assert (np.abs(lo.psum - hi.psum).astype(np.float64) <= ref.tol_psum_scaled(hi.psum, C, R)).all()
        assert (np.abs(lo.hsum - hi.hsum).astype(np.float64) <= ref.tol_hsum_scaled(hi.hsum, lo.count, C, R)).all()
        one = eref.new_state(S, C)
        ref.add_scaled(one, (x.astype(np.float64) / tau).astype(np.float32), 1.0)       # close to logits / tau, plainly added
        fin = one.count > 0
        assert np.allclose(one.psum[fin], lo.psum[fin], rtol=0, atol=1e-4)
    for tau in (0.0, -1.0, np.inf, np.nan):
        c = eref.new_state(S, C)
        assert ref.add_scaled(c, x, tau) == R * S and not c.count.any() and not c.bad.any()


@pytest.mark.parametrize("B", ref.STATS_B)
def test_stats_bins_equal_a_plain_loop_and_sums_inside_the_bounds(B):
    C = 5
    for n in ref.STATS_N:
        conf, label, target, prob = ref.stats_inputs(n, C, seed=n + B)
        lo = ref.stats(conf, label, target, prob, C, B)
        hi = ref.stats(conf, label, target, prob, C, B, np.longdouble)
        cnt, cor, cf = [0] * B, [0] * B, [0] * B
        used = []
        for i in range(n):
            c = float(conf[i])
            if label[i] < 0 or not 0 <= target[i] < C or not (0.0 <= c <= 1.0):
                continue
            used.append(i)
            b = min(B - 1, math.floor(c * B))
            cnt[b] += 1
            cor[b] += int(label[i] == target[i])
            cf[b] += round(c * 2 ** 32)         # (Python's round: to even, as llrint)
        assert lo.bin_count.tolist() == cnt and lo.bin_correct.tolist() == cor and lo.bin_conf.tolist() == cf
        assert lo.counts[0] == len(used) and lo.counts[:4].sum() == n
        # the order: used rows by descending confidence, ties by ascending row, then the rest by ascending row
        want = sorted(used, key=lambda i: (-float(conf[i]), i)) + [i for i in range(n) if i not in set(used)]
        assert lo.order.tolist() == want
        errs = [int(i in set(used) and label[i] != target[i]) for i in want]
        assert lo.err_prefix.tolist() == np.cumsum(errs).tolist() if n else True
        for f in ("bin_count", "bin_correct", "bin_conf", "counts", "order", "err_prefix"):
            assert (getattr(lo, f) == getattr(hi, f)).all(), f
        m = len(used)
        assert abs(float(lo.sums[0] - hi.sums[0])) <= ref.tol_stats_nll(hi.sums[0], n)
        assert abs(float(lo.sums[1] - hi.sums[1])) <= ref.tol_stats_brier(hi.sums[1], n, C)
        assert abs(float(lo.aurc - hi.aurc)) <= ref.tol_aurc(hi.aurc, m)
        if n >= 63:
            assert lo.counts[4] > 0 and lo.counts[1] > 0 and lo.counts[2] > 0 and lo.counts[3] > 0
        ece, mce = ref.ece_mce(lo.bin_count, lo.bin_correct, lo.bin_conf)
        assert 0.0 <= ece <= mce <= 1.0
