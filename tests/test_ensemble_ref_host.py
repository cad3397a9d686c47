"""The NumPy restatement of the ensemble kernels (tests/ensemble_ref.py) against torch in fp64, its bounds against a
long-double evaluation, and the GPU test's case table against pn_ensemble_route (a host-only query).  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import ensemble_ref as ref


def _route(rows, C):
    from pathnet_amd import _lib
    r = ctypes.c_int32(-7)
    rc = _lib.load().pn_ensemble_route(rows, C, ctypes.byref(r))
    return rc, r.value


@pytest.mark.parametrize("C,S,R", [(1, 5, 2), (2, 9, 3), (7, 40, 5), (65, 11, 2), (300, 3, 4)])
def test_reference_agrees_with_torch_fp64(C, S, R):
    x = ref.make_logits("normal", R, S, C, seed=C + S)
    st = ref.new_state(S, C)
    assert ref.add(st, x) == 0
    t = torch.from_numpy(x).double()
    p = torch.softmax(t, dim=2)
    logp = torch.log_softmax(t, dim=2)
    np.testing.assert_allclose(st.psum, p.sum(0).numpy(), rtol=0, atol=ref.tol_psum(st.psum, C, R).max())
    h = -(p * logp).sum(2).sum(0).numpy()
    assert (np.abs(st.hsum - h) <= ref.tol_hsum(st.hsum, st.count, C, R)).all()
    votes = torch.zeros(S, C, dtype=torch.int64)
    votes.scatter_add_(1, t.argmax(2).T.contiguous(), torch.ones(S, R, dtype=torch.int64))
    assert (st.votes == votes.numpy()).all() and (st.count == R).all() and (st.bad == 0).all()
    res = ref.finish(st)
    mean = p.mean(0)
    assert (res.label == mean.argmax(1).numpy()).all()
    assert (np.abs(res.prob - mean.float().numpy()) <= ref.ulp32(res.prob)).all()
    ent = -(mean * torch.log(mean)).sum(1).numpy()
    assert (np.abs(res.entropy - ent.astype(np.float32)) <= ref.ulp32(res.entropy) + 1e-12).all()


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("C,S,R", [(2, 30, 5), (7, 64, 2), (65, 20, 5), (1025, 6, 2)])
def test_bounds_hold_the_fp64_reference_with_room(kind, C, S, R):
    """the fp64 restatement against the same formulas in long double: within a TENTH of the derived bounds, so the bounds
    are not vacuous and the reference the kernels are compared with sits well inside them"""
    x = ref.make_logits(kind, R, S, C, seed=3)
    lo, hi = ref.new_state(S, C), ref.new_state(S, C, np.longdouble)
    ref.add(lo, x)
    ref.add(hi, x)
    for f in ("votes", "count", "bad"):
        assert (getattr(lo, f) == getattr(hi, f)).all(), f
    K = max(int(lo.count.max()), 1)
    e_p = np.abs(lo.psum - hi.psum).astype(np.float64)
    e_h = np.abs(lo.hsum - hi.hsum).astype(np.float64)
    assert (e_p <= 0.1 * ref.tol_psum(lo.psum, C, K)).all(), (e_p / ref.tol_psum(lo.psum, C, K)).max()
    assert (e_h <= 0.1 * ref.tol_hsum(lo.hsum, lo.count, C, K)).all(), (e_h / ref.tol_hsum(lo.hsum, lo.count, C, K)).max()
    a, b = ref.finish(lo), ref.finish(hi)
    rel_q = ref.rel_p(C) + (K + 1) * ref.U
    assert (np.abs(a.exact[0] - b.exact[0]) <= 0.1 * ref.tol_entropy(a.exact[0], C, rel_q)).all()


def test_reference_edge_rules():
    C = 4
    x = np.zeros((3, 6, C), np.float32)
    x[:, 0] = [1, 5, 5, 2]                  # tie: lowest index wins vote and label
    x[0, 1, 2] = np.nan                     # bad in one sample only
    x[:, 2, 1] = np.inf                     # bad in every sample
    x[:, 3] = [0, -800, 0, -1000]           # exact zeros: 0 log 0 = 0
    x[1, 4, 0] = -np.inf
    st = ref.new_state(8, C)
    index = np.array([7, 6, 5, 4, 3, 9], np.int32)     # the last one is outside
    assert ref.add(st, x, index) == 3
    assert st.count.tolist() == [0, 0, 0, 2, 3, 0, 2, 3] and st.bad.tolist() == [0, 0, 0, 1, 0, 3, 1, 0]
    assert st.votes[7].tolist() == [0, 3, 0, 0]
    assert st.psum[4].tolist() == [1.5, 0.0, 1.5, 0.0] and st.hsum[4] == pytest.approx(3 * np.log(2))
    target = np.array([0, 1, 2, 3, -1, C, 0, 1], np.int64)
    res = ref.finish(st, target=target)
    assert res.label.tolist() == [-1, -1, -1, 0, 0, -1, 0, 1]
    assert res.skipped.tolist() == [2, 4] and res.confusion.sum() == 3
    assert res.confusion[3, 0] == 1 and res.confusion[0, 0] == 1 and res.confusion[1, 1] == 1
    assert (res.prob[[0, 1, 2, 5]] == 0).all() and (res.entropy[[0, 1, 2, 5]] == 0).all()
    sub = ref.finish(st, subset=np.array([7, 7, -1, 8, 4], np.int32), target=target)
    assert sub.label.tolist() == [1, 1, -1, -1, 0] and sub.skipped.tolist() == [1, 2]
    assert (sub.mutual_info >= 0).all() and sub.agreement.tolist() == [1, 1, 0, 0, 1]


def test_case_table_covers_every_route_and_boundary():
    from pathnet_amd import _lib
    assert (ref.ROUTE_NONE, ref.ROUTE_THREAD, ref.ROUTE_WAVE, ref.ROUTE_BLOCK) == (
        _lib.ENSEMBLE_ROUTE_NONE, _lib.ENSEMBLE_ROUTE_THREAD, _lib.ENSEMBLE_ROUTE_WAVE, _lib.ENSEMBLE_ROUTE_BLOCK)
    cases = ref.case_table()
    assert {c for c, _, _ in cases} >= set(ref.C_VALUES) | set(ref.BOUNDARY_C)
    assert {s for _, s, _ in cases} >= set(ref.S_VALUES) and {r for _, _, r in cases} == set(ref.R_VALUES)
    seen = set()
    for C, S, _ in cases:
        rc, got = _route(S, C)
        assert rc == 0 and got == ref.route(S, C), (C, S, got)
        seen.add(got)
    assert seen == {ref.ROUTE_NONE, ref.ROUTE_THREAD, ref.ROUTE_WAVE, ref.ROUTE_BLOCK}
    # the boundaries the library has are exactly the ones the table names: walk all C, note every change of route
    changes = [C for C in range(2, ref.MAX_CLASSES + 1) if _route(5, C)[1] != _route(5, C - 1)[1]]
    assert changes == [17, 1025]
    for C in changes:
        assert {C - 1, C} <= {c for c, s, _ in cases if s > 0}
    # ... and none in rows, besides rows == 0
    assert {_route(rows, 7)[1] for rows in (1, 2, 63, 64, 65, 255, 256, 257, 65536 * 4 + 1, 2 ** 31 - 1)} == {ref.ROUTE_THREAD}
    assert _route(0, 7)[1] == ref.ROUTE_NONE and _route(1, 7)[1] == ref.ROUTE_THREAD


def test_limits_are_refused_without_a_device():
    from pathnet_amd import _lib
    lib = _lib.load()
    n = ctypes.c_int64(-1)
    assert lib.pn_ensemble_state_bytes(10, 7, ctypes.byref(n)) == 0 and n.value == 10 * (12 * 7 + 16)
    assert lib.pn_ensemble_state_bytes(0, 1, ctypes.byref(n)) == 0 and n.value == 0
    for rows, C in ((1, 0), (1, 4097), (-1, 3), (2 ** 31, 3)):
        assert lib.pn_ensemble_state_bytes(rows, C, ctypes.byref(n)) == _lib.PN_ERR_ARG
        assert _route(rows, C)[0] == _lib.PN_ERR_ARG
    # argument errors of add / finish come before any device call: they are answered here, without a GPU
    out = _lib.EnsembleOut()
    assert lib.pn_ensemble_add(None, None, 0, 1, 3, None, 1, None, None, None) == _lib.PN_ERR_ARG       # R = 0
    assert lib.pn_ensemble_add(None, None, 1, 5, 3, None, 4, None, None, None) == _lib.PN_ERR_ARG       # S > rows, no index
    assert lib.pn_ensemble_add(None, None, 1, 2, 5000, None, 4, None, None, None) == _lib.PN_ERR_ARG
    assert lib.pn_ensemble_finish(None, 4, 3, None, None, 0, None, None, None) == _lib.PN_ERR_ARG       # no out
    assert lib.pn_ensemble_finish(None, 4, 3, None, None, 2, None, ctypes.byref(out), None) == _lib.PN_ERR_ARG
    out.skipped = 8
    assert lib.pn_ensemble_finish(None, 4, 3, None, None, 0, None, ctypes.byref(out), None) == _lib.PN_ERR_ARG


def test_metrics_from_confusion_is_classification_metrics():
    from pathnet_amd import trainer
    g = torch.Generator().manual_seed(4)
    for C in (2, 5, 9):
        y = torch.randint(0, C, (200,), generator=g)
        p = torch.where(torch.rand(200, generator=g) < 0.6, y, torch.randint(0, C - 1, (200,), generator=g))
        conf = torch.bincount(y * C + p, minlength=C * C).view(C, C)
        assert trainer.metrics_from_confusion(conf) == trainer.classification_metrics(y, p, C)
