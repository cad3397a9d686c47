"""pn_calib_sweep, pn_ensemble_add_scaled and pn_calib_stats on the GPU, through the C ABI, against the NumPy restatement
tests/calib_ref.py.

As in test_gpu_ensemble.py every input, state, workspace and output sits between two guard bands of 0xFF bytes that must come
back untouched, and outputs start as 0xFF themselves.

Held to (bounds and their derivation: calib_ref's docstring): best, tau, counts, the bin arrays, order and err_prefix
exactly; row_nll element by element and nll within the derived fp64 bound of the long-double evaluation; the scaled state
bit-equal to the plain add's at tau = 1.0 and within the bound elsewhere; nll, brier and aurc sums within their bounds.
"""
import ctypes

import numpy as np
import pytest
import torch

import calib_ref as ref
import ensemble_ref as eref
import test_gpu_ensemble as tge

pytestmark = pytest.mark.gpu

Guarded, lib_ctx = tge.Guarded, tge.lib_ctx


def guarded_of(a):
    a = np.ascontiguousarray(a)
    g = Guarded(a.nbytes)
    g.payload.copy_(torch.from_numpy(a.view(np.uint8).reshape(-1)))
    return g


def gpu_sweep(x, y, temps):
    """-> (dict of numpy outputs incl. row_nll, the raw bytes of everything written)"""
    _lib, lib, ctx, stream = lib_ctx()
    R, S, C = x.shape
    T = len(temps)
    need = ctypes.c_int64(-1)
    _lib.check(lib.pn_calib_sweep_workspace_bytes(S, T, ctypes.byref(need)))
    assert need.value >= 8 * S * T and need.value % 8 == 0
    xg, yg, tg = guarded_of(x), guarded_of(np.asarray(y, np.int64)), guarded_of(np.asarray(temps, np.float64))
    ws = Guarded(need.value)
    bufs = dict(nll=Guarded(8 * T), best=Guarded(4), tau=Guarded(8), counts=Guarded(24))
    out = _lib.CalibSweepOut(*(bufs[k].ptr() for k in _lib.CalibSweepOut.FIELDS))
    _lib.check(lib.pn_calib_sweep(ctx, xg.ptr(), R, S, C, yg.ptr(), tg.ptr(), T, ws.ptr(), need.value, ctypes.byref(out),
                                  stream))
    torch.cuda.synchronize()
    for g in (xg, yg, tg, ws) + tuple(bufs.values()):
        assert g.intact()
    got = dict(nll=bufs["nll"].numpy(np.float64, (T,)), best=int(bufs["best"].numpy(np.int32, (1,))[0]),
               tau=float(bufs["tau"].numpy(np.float64, (1,))[0]), counts=bufs["counts"].numpy(np.int64, (3,)),
               row_nll=ws.payload[:8 * S * T].cpu().numpy().view(np.float64).reshape(S, T).copy())
    raw = torch.cat([bufs[k].payload for k in ("nll", "best", "tau", "counts")] + [ws.payload[:8 * S * T]]).clone()
    return got, raw


def check_sweep(got, x, y, temps, case):
    C, S, R, T = case
    lo, hi = ref.sweep(x, y, temps), ref.sweep(x, y, temps, np.longdouble)
    ok, ratio = ref.decidable(lo, hi, C, R)
    assert ok, "%s: best hangs on a rounding (%g x the bound)" % (case, ratio)
    assert (got["counts"] == lo.counts).all(), (case, got["counts"], lo.counts)
    tol_rows = ref.tol_row_nll(hi.q, C, R)
    want = hi.row_nll.astype(np.float64)
    same_inf = np.isinf(want) & (got["row_nll"] == want)
    with np.errstate(invalid="ignore"):
        err = np.where(same_inf, 0.0, np.abs(got["row_nll"] - want))
    assert (err <= tol_rows).all(), "%s: row_nll off by %g of its bound" % (case, (err / tol_rows).max())
    fin = np.isfinite(hi.nll.astype(np.float64))
    assert (np.isfinite(got["nll"]) == fin).all() and (got["nll"][~fin] == np.inf).all(), case
    e_nll = np.abs(got["nll"][fin] - hi.nll[fin].astype(np.float64))
    tol = ref.tol_nll(want, tol_rows)[fin]
    assert (e_nll <= tol).all(), "%s: nll off by %g of its bound" % (case, (e_nll / tol).max())
    assert got["best"] == lo.best and got["tau"] == lo.tau, (case, got["best"], lo.best)


@pytest.mark.parametrize("kind", ref.SWEEP_KINDS)
def test_sweep_case_table(kind):
    """every (C, S, R, T) of the table: row_nll, nll, best, tau and counts against the restatement; a second run bit-equal to
    the first; a run on permuted rows equal to the first row for row"""
    for case in ref.sweep_cases(kind):
        C, S, R, T = case
        x, y, temps = ref.sweep_inputs(kind, case)
        got, raw = gpu_sweep(x, y, temps)
        check_sweep(got, x, y, temps, case)
        again, raw2 = gpu_sweep(x, y, temps)
        assert torch.equal(raw, raw2), "%s: two runs differ" % (case,)
        if S > 1:
            perm = np.random.default_rng(S).permutation(S)
            moved, _ = gpu_sweep(x[:, perm], y[perm], temps)
            assert (moved["row_nll"].view(np.int64) == got["row_nll"][perm].view(np.int64)).all(), case
            assert (moved["counts"] == got["counts"]).all() and moved["best"] == got["best"]
        if S == 0:
            assert got["best"] == -1 and got["tau"] == 1.0 and not got["counts"].any()


def test_sweep_refuses_bad_shapes_before_any_device_call():
    _lib, lib, ctx, stream = lib_ctx()
    n = ctypes.c_int64(-7)
    for S, T in ((-1, 3), (2 ** 31, 3), (5, 0), (5, 257)):
        assert lib.pn_calib_sweep_workspace_bytes(S, T, ctypes.byref(n)) == _lib.PN_ERR_ARG and n.value == -7
    g = Guarded(4096)
    out_bufs = dict(nll=Guarded(64), best=Guarded(4), tau=Guarded(8), counts=Guarded(24))
    out = _lib.CalibSweepOut(*(out_bufs[k].ptr() for k in _lib.CalibSweepOut.FIELDS))
    call = lambda R, S, C, T, ws_bytes, o=out: lib.pn_calib_sweep(ctx, g.ptr(), R, S, C, g.ptr(), g.ptr(), T, g.ptr(),    # noqa: E731
                                                                  ws_bytes, ctypes.byref(o) if o is not None else None, stream)
    for args in ((0, 4, 3, 2, 4096), (1, -1, 3, 2, 4096), (1, 4, 0, 2, 4096), (1, 4, 4097, 2, 4096), (1, 4, 3, 0, 4096),
                 (1, 4, 3, 257, 4096), (1, 4, 3, 2, 8)):
        assert call(*args) == _lib.PN_ERR_ARG, args
    assert call(1, 4, 3, 2, 4096, None) == _lib.PN_ERR_ARG
    torch.cuda.synchronize()
    assert g.untouched() and all(b.untouched() for b in out_bufs.values())


# ---- scaled add -------------------------------------------------------------------------------------------------------------
def gpu_add_scaled(state, x, rows, tau, index=None, status=None):
    _lib, lib, ctx, stream = lib_ctx()
    R, S, C = x.shape
    xg, tg = guarded_of(x), guarded_of(np.array([tau], np.float64))
    ig = guarded_of(np.asarray(index, np.int32)) if index is not None else None
    _lib.check(lib.pn_ensemble_add_scaled(ctx, xg.ptr(), R, S, C, ig.ptr() if ig is not None else None, rows, state.ptr(),
                                          status.ptr() if status is not None else None, tg.ptr(), stream))
    torch.cuda.synchronize()
    assert xg.intact() and tg.intact() and (ig is None or ig.intact()) and state.intact()


SCALED_SHAPES = ((1, 9, 2), (7, 130, 3), (16, 65, 2), (17, 65, 2), (65, 33, 5), (1024, 5, 2), (1025, 5, 2), (4096, 3, 1))


@pytest.mark.parametrize("kind", ("normal", "nonfinite", "ties"))
def test_scaled_add_at_unit_temperature_leaves_the_plain_bits(kind):
    """all three routes (C <= 16, <= 1024, above), with and without an index"""
    for C, S, R in SCALED_SHAPES:
        x = eref.make_logits(kind, R, S, C, seed=C + S)
        for rows, index in ((S, None), (S + 5, np.random.default_rng(C).permutation(S + 5)[:S].astype(np.int32))):
            nb = tge.state_bytes(rows, C)
            plain, scaled = Guarded(nb, fill=0), Guarded(nb, fill=0)
            tge.gpu_add(plain, x, rows, index)
            gpu_add_scaled(scaled, x, rows, 1.0, index)
            assert torch.equal(plain.payload, scaled.payload), (kind, C, S, R)


@pytest.mark.parametrize("tau", (0.37, 2.5))
def test_scaled_add_inside_the_bound(tau):
    for C, S, R in SCALED_SHAPES:
        for kind in ("normal", "nonfinite"):
            x = eref.make_logits(kind, R, S, C, seed=3 * C + S)
            state = Guarded(tge.state_bytes(S, C), fill=0)
            gpu_add_scaled(state, x[:1], S, tau)
            if R > 1:
                gpu_add_scaled(state, x[1:], S, tau)           # two calls: the state accumulates in ascending r
            got = tge.read_state(state, S, C)
            lo, hi = eref.new_state(S, C), eref.new_state(S, C, np.longdouble)
            ref.add_scaled(lo, x, tau)
            ref.add_scaled(hi, x, tau)
            for f in ("votes", "count", "bad"):
                assert (getattr(got, f) == getattr(lo, f)).all(), (f, C, S, R)
            e_p = np.abs(got.psum - hi.psum).astype(np.float64)
            tol = ref.tol_psum_scaled(hi.psum.astype(np.float64), C, R)
            assert (e_p <= tol).all(), "psum off by %g of its bound" % (e_p / tol).max()
            e_h = np.abs(got.hsum - hi.hsum).astype(np.float64)
            tol = ref.tol_hsum_scaled(hi.hsum.astype(np.float64), lo.count, C, R)
            assert (e_h <= tol).all(), "hsum off by %g of its bound" % (e_h / tol).max()


def test_scaled_add_refuses_a_bad_temperature():
    for C, S, R in ((7, 70, 3), (65, 9, 2), (1025, 3, 2)):
        x = eref.make_logits("normal", R, S, C, seed=1)
        for tau in (0.0, -1.0, np.inf, -np.inf, np.nan):
            state, status = Guarded(tge.state_bytes(S, C)), Guarded(4, fill=0)
            gpu_add_scaled(state, x, S, tau, status=status)
            assert state.untouched() and status.intact(), (C, tau)
            assert status.numpy(np.int32, (1,))[0] == R * S
        state = Guarded(tge.state_bytes(S, C))
        gpu_add_scaled(state, x, S, np.nan)                    # a NULL status is fine
        assert state.untouched()
    _lib, lib, ctx, stream = lib_ctx()
    g = Guarded(4096)
    assert lib.pn_ensemble_add_scaled(ctx, g.ptr(), 1, 4, 3, None, 4, g.ptr(), None, None, stream) == _lib.PN_ERR_ARG
    assert g.untouched()


# ---- statistics -------------------------------------------------------------------------------------------------------------
def gpu_stats(conf, label, target, prob, C, B, curve=True, acc=None):
    """one pn_calib_stats; acc: the Guarded accumulators of an earlier call to add to -> (dict of numpy, accumulators)"""
    _lib, lib, ctx, stream = lib_ctx()
    n = len(conf)
    need = ctypes.c_int64(-1)
    _lib.check(lib.pn_calib_stats_workspace_bytes(n, B, ctypes.byref(need)))
    ins = [guarded_of(np.asarray(conf, np.float32)), guarded_of(np.asarray(label, np.int64)),
           guarded_of(np.asarray(target, np.int64)), guarded_of(np.asarray(prob, np.float32)) if prob is not None else None]
    ws = Guarded(need.value)
    if acc is None:
        acc = dict(bin_count=Guarded(8 * B, fill=0), bin_correct=Guarded(8 * B, fill=0), bin_conf=Guarded(8 * B, fill=0),
                   counts=Guarded(40, fill=0), sums=Guarded(16, fill=0))
    bufs = dict(acc)
    if curve:
        bufs.update(order=Guarded(4 * n), err_prefix=Guarded(4 * n), aurc=Guarded(8))
    out = _lib.CalibStatsOut(*(bufs[k].ptr() if k in bufs else None for k in _lib.CalibStatsOut.FIELDS))
    _lib.check(lib.pn_calib_stats(ctx, ins[0].ptr(), ins[1].ptr(), ins[2].ptr(), ins[3].ptr() if ins[3] is not None else None,
                                  n, C, B, ws.ptr(), need.value, ctypes.byref(out), stream))
    torch.cuda.synchronize()
    for g in [i for i in ins if i is not None] + [ws] + list(bufs.values()):
        assert g.intact()
    shapes = dict(bin_count=(np.int64, (B,)), bin_correct=(np.int64, (B,)), bin_conf=(np.int64, (B,)), counts=(np.int64, (5,)),
                  sums=(np.float64, (2,)), order=(np.int32, (n,)), err_prefix=(np.int32, (n,)), aurc=(np.float64, (1,)))
    return {k: g.numpy(*shapes[k]) for k, g in bufs.items()}, acc


def check_stats(got, want, hi, n, C, with_prob=True):
    for f in ("bin_count", "bin_correct", "bin_conf"):
        assert (got[f] == getattr(want, f)).all(), f
    assert (got["counts"] == want.counts).all(), (got["counts"], want.counts)
    if "order" in got:
        assert (got["order"] == want.order).all() and (got["err_prefix"] == want.err_prefix).all()
        assert abs(got["aurc"][0] - float(hi.aurc)) <= ref.tol_aurc(hi.aurc, int(want.counts[0]))
    if with_prob:
        assert abs(got["sums"][0] - float(hi.sums[0])) <= ref.tol_stats_nll(hi.sums[0], n)
        assert abs(got["sums"][1] - float(hi.sums[1])) <= ref.tol_stats_brier(hi.sums[1], n, C)
    else:
        assert (got["sums"] == 0).all()


@pytest.mark.parametrize("B", ref.STATS_B)
def test_stats_case_table(B):
    C = 5
    for n in ref.STATS_N:
        conf, label, target, prob = ref.stats_inputs(n, C, seed=n + B)
        want = ref.stats(conf, label, target, prob, C, B)
        hi = ref.stats(conf, label, target, prob, C, B, np.longdouble)
        got, _ = gpu_stats(conf, label, target, prob, C, B)
        check_stats(got, want, hi, n, C)
        again, _ = gpu_stats(conf, label, target, prob, C, B)
        for k in got:
            assert (got[k].view(np.uint8) == again[k].view(np.uint8)).all(), "%s: two runs differ" % k
        if n == 0:
            assert got["aurc"][0] == 0.0 and not got["bin_count"].any()


def test_stats_optional_parts_and_wide_rows():
    """without prob and without the curve nothing of them is written; C past one cache line and C = 1"""
    for C, n, B in ((1, 70, 4), (130, 300, 15), (4096, 9, 16)):
        conf, label, target, prob = ref.stats_inputs(n, C, seed=C)
        want = ref.stats(conf, label, target, prob, C, B)
        hi = ref.stats(conf, label, target, prob, C, B, np.longdouble)
        got, _ = gpu_stats(conf, label, target, prob, C, B)
        check_stats(got, want, hi, n, C)
        bare, _ = gpu_stats(conf, label, target, None, C, B, curve=False)
        assert set(bare) == {"bin_count", "bin_correct", "bin_conf", "counts", "sums"}
        no_prob = ref.stats(conf, label, target, None, C, B)
        check_stats(bare, no_prob, no_prob, n, C, with_prob=False)


def test_stats_bins_accumulate_across_calls():
    C, B, n = 5, 16, 700
    conf, label, target, prob = ref.stats_inputs(n, C, seed=4)
    whole, _ = gpu_stats(conf, label, target, prob, C, B, curve=False)
    cut = 257
    first, acc = gpu_stats(conf[:cut], label[:cut], target[:cut], prob[:cut], C, B, curve=False)
    both, _ = gpu_stats(conf[cut:], label[cut:], target[cut:], prob[cut:], C, B, curve=False, acc=acc)
    for f in ("bin_count", "bin_correct", "bin_conf", "counts"):
        assert (both[f] == whole[f]).all(), f
    hi = ref.stats(conf, label, target, prob, C, B, np.longdouble)
    assert abs(both["sums"][0] - float(hi.sums[0])) <= 2 * ref.tol_stats_nll(hi.sums[0], n)
    assert abs(both["sums"][1] - float(hi.sums[1])) <= 2 * ref.tol_stats_brier(hi.sums[1], n, C)


def test_stats_refuses_bad_shapes_before_any_device_call():
    _lib, lib, ctx, stream = lib_ctx()
    n = ctypes.c_int64(-7)
    for rows, B in ((-1, 15), (5, 0), (5, 1025)):
        assert lib.pn_calib_stats_workspace_bytes(rows, B, ctypes.byref(n)) == _lib.PN_ERR_ARG and n.value == -7
    g = Guarded(1 << 16)
    full = _lib.CalibStatsOut(*(g.ptr() for _ in _lib.CalibStatsOut.FIELDS))
    no_bins = _lib.CalibStatsOut(None, g.ptr(), g.ptr(), None, g.ptr(), None, None, None)
    no_sums = _lib.CalibStatsOut(g.ptr(), g.ptr(), g.ptr(), None, None, None, None, None)
    no_order = _lib.CalibStatsOut(g.ptr(), g.ptr(), g.ptr(), None, g.ptr(), None, g.ptr(), None)
    call = lambda rows, C, B, ws_bytes, o: lib.pn_calib_stats(ctx, g.ptr(), g.ptr(), g.ptr(), g.ptr(), rows, C, B, g.ptr(),   # noqa: E731
                                                              ws_bytes, ctypes.byref(o), stream)
    for args in ((-1, 3, 15, 1 << 16, full), (4, 0, 15, 1 << 16, full), (4, 4097, 15, 1 << 16, full), (4, 3, 0, 1 << 16, full),
                 (4, 3, 1025, 1 << 16, full), (4, 3, 15, 64, full), (4, 3, 15, 1 << 16, no_bins), (4, 3, 15, 1 << 16, no_sums),
                 (4, 3, 15, 1 << 16, no_order)):
        assert call(*args) == _lib.PN_ERR_ARG, args[:4]
    torch.cuda.synchronize()
    assert g.untouched()


def test_python_layer_matches_the_abi():
    """fit_temperature (both rounds), Ensemble(temperature=) with a device tau, Prediction.calibration and threshold()"""
    import pathnet_amd
    case = (7, 256, 2, 25)
    S = case[1]
    x, y, temps = ref.sweep_inputs("base", case)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    assert np.allclose(pathnet_amd.calibration.DEFAULT_GRID, ref.DEFAULT_GRID, rtol=1e-15, atol=0)
    assert int(pathnet_amd.fit_temperature(xt, yt, rounds=1).best) == ref.sweep(x, y, ref.DEFAULT_GRID).best
    one = pathnet_amd.fit_temperature(xt, yt, grid=ref.DEFAULT_GRID, rounds=1)
    want = ref.sweep(x, y, ref.DEFAULT_GRID)
    s = one.summary()
    assert s["best"] == want.best and s["tau"] == want.tau and s["rows_used"] == S
    assert np.allclose(s["nll"], want.nll, rtol=1e-12) and s["grid"] == ref.DEFAULT_GRID.tolist()
    two = pathnet_amd.fit_temperature(xt, yt, grid=ref.DEFAULT_GRID)
    fine = two.temps.cpu().numpy()
    lo, hi = ref.DEFAULT_GRID[max(want.best - 1, 0)], ref.DEFAULT_GRID[min(want.best + 1, 24)]
    assert len(fine) == 17 and fine[0] == lo and np.allclose(fine, lo * (hi / lo) ** (np.arange(17) / 16), rtol=1e-14)
    again = ref.sweep(x, y, fine)
    assert int(two.best) == again.best and float(two.tau) == again.tau == fine[again.best]
    assert float(two.nll.min()) <= float(one.nll.min()) * (1 + 1e-12)       # (the fine grid straddles the coarse best point)
    # the device tau drives the ensemble
    ens = pathnet_amd.Ensemble(S, 7, "cuda", temperature=two.tau).add(xt)
    st = eref.new_state(S, 7)
    ref.add_scaled(st, x, again.tau)
    assert (np.abs(ens.psum.cpu().numpy() - st.psum) <= 2 * ref.tol_psum_scaled(st.psum, 7, 2)).all()
    plain = pathnet_amd.Ensemble(S, 7, "cuda").add(xt)
    unit = pathnet_amd.Ensemble(S, 7, "cuda", temperature=1.0).add(xt)
    assert torch.equal(plain.state, unit.state)
    with pytest.raises(ValueError):
        pathnet_amd.Ensemble(4, 3, "cuda", temperature=torch.ones(2))
    # calibration of the prediction against the restatement fed the read-back prediction
    pred = ens.result()
    for bins, curve in ((15, True), (4, False)):
        cal = pred.calibration(yt, bins=bins, curve=curve)
        conf, label, prob = (t.cpu().numpy() for t in (pred.confidence, pred.label, pred.prob))
        w = ref.stats(conf, label, y, prob, 7, bins)
        assert (cal.bin_count.cpu().numpy() == w.bin_count).all() and (cal.bin_conf.cpu().numpy() == w.bin_conf).all()
        summ = cal.summary()
        ece, mce = ref.ece_mce(w.bin_count, w.bin_correct, w.bin_conf)
        m = int(w.counts[0])
        assert summ["used"] == m == S and summ["ece"] == pytest.approx(ece, rel=1e-12, abs=1e-15)
        assert summ["mce"] == pytest.approx(mce, rel=1e-12) and summ["nll"] == pytest.approx(float(w.sums[0]) / (m - w.counts[4]), rel=1e-12)
        assert summ["brier"] == pytest.approx(float(w.sums[1]) / m, rel=1e-12)
        assert summ["accuracy"] == pytest.approx(w.bin_correct.sum() / m)
        if curve:
            assert (cal.order.cpu().numpy() == w.order).all() and summ["aurc"] == pytest.approx(float(w.aurc), rel=1e-12)
            for cov in (0.1, 0.5, 1.0):
                k = int(np.ceil(cov * m))
                assert float(cal.threshold(cov)) == conf[w.order[k - 1]]
        else:
            assert cal.order is None and cal.aurc is None and "aurc" not in summ
            with pytest.raises(ValueError):
                cal.threshold(0.5)
    with pytest.raises(pathnet_amd._lib.PnError):
        pred.calibration(yt, bins=2000)
