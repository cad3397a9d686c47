"""The NumPy restatement of pn_explain_groups / pn_explain_totals (tests/explain_ref.py) against the fp64 reference of the
weighted pooling (tests/weighted_pool_ref.py), its edge rules, and its bound functions.  No GPU."""
import numpy as np
import pytest
import torch

from oracle import pagg_oracle as po
import explain_ref as ref
import weighted_pool_ref as wref
from test_path_weights_cpu import N, F, H, C, L, params_for, paths

S, W = 6, 5
TOL = 1e-10     # both sides are fp64 with sums of <= 8 terms of size O(1): five orders above their rounding, five below the
                # kernel's fp32 tolerance


@pytest.mark.parametrize("norm", ["sum", "count"])
@pytest.mark.parametrize("variant", po.VARIANTS)
def test_drop_and_keep_are_the_weighted_forward(variant, norm):
    """drop_g = the library's forward with the members of R given weight 0, keep_g = with everything else given weight 0:
    every group of "path", a grouping with two-member groups, with and without caller weights that hold a dead member"""
    rng = np.random.default_rng(7)
    p, X = params_for(variant, rng), torch.as_tensor(rng.uniform(0, 1, (N, F)))
    sel, ids, codes = paths(rng, S, W)
    hg = ref.member_states(variant, p, X, ids, codes, sel, W, L)
    fc2_w, fc2_b = p["fc2.weight"].numpy(), p["fc2.bias"].numpy()
    caller = rng.choice([0.5, 1.0, 2.0], (S, W))
    caller[:, 1] = 0.0                                  # a dead member in every row
    caller[2, 3] = np.nan
    by_path = np.tile(np.arange(W), (S, 1))
    pairs = by_path // 2                                # groups {0, 1}, {2, 3}, {4}
    for gm in (None, caller):
        base = np.ones((S, W)) if gm is None else gm
        logits, emb, coef = wref.forward(variant, p, X, ids, codes, sel, W, L, wref.to_slots(variant, base), norm)
        for group, G in ((by_path, W), (pairs, 3)):
            res = ref.groups(hg, coef.numpy(), emb[:, :H].numpy(), fc2_w, fc2_b, gm, group, G,
                             ref.NORM_SUM if norm == "sum" else ref.NORM_COUNT, variant == "hetero", in_dtype=np.float64)
            assert np.abs(res.full - logits.numpy()).max() < TOL
            for g in range(G):
                R = group == g
                for name, omega in (("drop_logits", np.where(R, 0.0, base)), ("keep_logits", np.where(R, base, 0.0))):
                    want, _, _ = wref.forward(variant, p, X, ids, codes, sel, W, L, wref.to_slots(variant, omega), norm)
                    got = getattr(res, name)[:, g]
                    assert np.abs(got - want.numpy()).max() < TOL, (name, g, gm is None)
            assert (res.present == np.stack([(wref.live(base).numpy() > 0)[:, group[0] == g].sum(1) for g in range(G)], 1)).all()


def tiny(seed=0, S=4, W=4, H=5, C=3):
    rng = np.random.default_rng(seed)
    return dict(state=rng.standard_normal((S, W, H)).astype(np.float32), coef=(rng.random((S, W)) + 0.5).astype(np.float32),
                ego=rng.standard_normal((S, H)).astype(np.float32), fc2_w=rng.standard_normal((C, 2 * H)).astype(np.float32),
                fc2_b=rng.standard_normal(C).astype(np.float32))


def test_edge_rules():
    d = tiny()
    S, W, C = 4, 4, 3
    group = np.array([[0, 0, 1, 5]] * S)                  # group 2 is empty, member 3 belongs to no group
    weight = np.ones((S, W), np.float32)
    weight[1] = [1, 0, 0, 0]                              # row 1: a single live member, in group 0
    weight[2] = [0, 0, 0, 0]                              # row 2: nothing live
    d = dict(d, coef=d["coef"] * (weight > 0))            # (the coefficient the library reports for a dead member is 0)
    for norm in (ref.NORM_SUM, ref.NORM_COUNT):
        for renorm in (0, 1):
            r = ref.groups(**d, weight=weight, group=group, G=3, norm=norm, renorm=renorm, target=np.array([0, 1, 2, 1]))
            # an empty group: drop = full bit for bit, rho_d = 1 exactly, keep = e, never a flip
            assert (r.drop_logits[:, 2] == r.full).all() and (r.rho_d[:, 2] == 1.0).all()
            assert (r.keep_logits[:, 2] == r.e).all() and (r.flip[:, 2] == 0).all() and (r.present[:, 2] == 0).all()
            assert (r.drop_delta[:, 2] == 0).all() and (r.keep_gain[:, 2] == 0).all()
            # the group that holds every live member: dropping it leaves e; keeping it is the full row
            assert (r.drop_logits[1, 0] == r.e[1]).all() and r.rho_d[1, 0] == 0
            assert np.abs(r.keep_logits[1, 0] - r.full[1]).max() < 1e-12
            assert r.present[1].tolist() == [1, 0, 0] and r.present[2].tolist() == [0, 0, 0]
            # nothing live: every vector is e
            assert (r.drop_logits[2] == r.e[2]).all() and (r.keep_logits[2] == r.e[2]).all()
            # the member of no group is never removed and never kept alone
            assert r.present[0].tolist() == [2, 1, 0]
            if norm == ref.NORM_COUNT and not renorm:
                # (applied as given and nothing renormalised: the two parts of row 0 add up to the whole)
                assert np.abs(r.drop_logits[0, 0] + r.keep_logits[0, 0] - r.e[0] - r.full[0]).max() < 1e-12
    # K_rest == 0 under renorm: the pooled part is zero
    d2 = dict(d, coef=d["coef"].copy())
    d2["coef"][0, 2:] = 0.0
    r = ref.groups(**d2, weight=None, group=group, G=3, norm=ref.NORM_SUM, renorm=1)
    assert (r.drop_logits[0, 0] == r.e[0]).all() and r.rho_d[0, 0] == 0
    assert (r.keep_logits[0, 1] == r.e[0]).all() and r.rho_k[0, 1] == 0          # K_R == 0 likewise
    r0 = ref.groups(**d2, weight=None, group=group, G=3, norm=ref.NORM_SUM, renorm=0)
    assert r0.rho_d[0, 0] == 2.0 and r0.rho_k[0, 1] == 4.0     # (without renorm the rule does not apply)
    # without a target: the argmax of full, and lp(full) is then the largest log-probability
    assert (r.target_used == r.full.argmax(1)).all() and r.status.tolist() == [0, 0]
    # a target out of range: zeros, no flips, counted; the logits are still there
    r = ref.groups(**d, weight=None, group=group, G=3, norm=ref.NORM_SUM, renorm=0, target=np.array([0, C, -1, 2]))
    assert r.status.tolist() == [2, 0] and (r.drop_delta[1:3] == 0).all() and (r.keep_gain[1:3] == 0).all()
    assert (r.flip[1:3] == 0).all() and np.isfinite(r.drop_logits).all() and r.target_used.tolist() == [0, C, -1, 2]
    # a bad row: NaN floats, no flip, present still counted, and it is not counted as a bad target
    d3 = dict(d, state=d["state"].copy())
    d3["state"][3, 2, 4] = np.inf
    r = ref.groups(**d3, weight=None, group=group, G=3, norm=ref.NORM_SUM, renorm=0, target=np.array([0, 1, 2, 7]))
    assert r.status.tolist() == [0, 1] and r.present[3].tolist() == [2, 1, 0] and (r.flip[3] == 0).all()
    for k in ("full", "contribution", "drop_logits", "keep_logits", "drop_delta", "keep_gain"):
        a = getattr(r, k)
        assert np.isnan(a[3]).all() and np.isfinite(a[:3]).all(), k


def test_bounds_are_not_trivial():
    """longdouble against the fp64 restatement sits inside every bound, and the bounds are far below the fp32 ulp they are
    added to"""
    if np.finfo(np.longdouble).nmant <= 52:
        pytest.skip("long double is double here")
    for sh in ({"S": 5, "W": 5, "H": 32, "C": 3, "G": 3}, {"S": 3, "W": 40, "H": 128, "C": 7, "G": 40}):
        for renorm in (0, 1):
            case = ref.make_case(seed=3, renorm=renorm, **sh)
            lo, hi = ref.run(case), ref.run(case, np.longdouble)
            assert (lo.flip == hi.flip).all() and (lo.present == hi.present).all() and (lo.target_used == hi.target_used).all()
            for k, tol in hi.tol.items():
                err = np.abs(getattr(lo, k).astype(np.longdouble) - getattr(hi, k)).astype(np.float64)
                assert (err <= tol).all(), (k, (err / tol).max())
                assert tol.max() < 1e-9, k
            assert np.abs(lo.drop_delta).max() > 1e-3           # and the scores are not all tiny


def test_totals_are_exact_on_integers_and_split_calls_follow_the_sequence():
    case = ref.make_case(S=40, W=5, H=8, C=3, G=4, seed=5)
    r = ref.run(case)
    dd, kg = ref.f32(r.drop_delta), ref.f32(r.keep_gain)
    dd[7, 1] = np.nan                                       # a row that is left out of group 1
    one = ref.totals_add(ref.new_totals(4), dd, kg, r.flip, r.present)
    ok = (r.present > 0) & np.isfinite(dd) & np.isfinite(kg)
    assert (one.rows_present == ok.sum(0)).all() and (one.members == (r.present * ok).sum(0)).all()
    assert (one.flips == (r.flip * ok).sum(0)).all()
    hi = ref.totals_add(ref.new_totals(4, np.longdouble), dd, kg, r.flip, r.present)
    for a, b, v in ((one.drop_delta_sum, hi.drop_delta_sum, dd), (one.keep_gain_sum, hi.keep_gain_sum, kg)):
        bound = ref.tol_totals(np.where(ok, np.abs(v), 0).sum(0), 40)
        assert (np.abs(a - b).astype(np.float64) <= bound).all() and bound.max() < 1e-12
    two = ref.new_totals(4)
    ref.totals_add(two, dd, kg, r.flip, r.present, rows=np.arange(20))
    ref.totals_add(two, dd, kg, r.flip, r.present, rows=np.arange(20, 40))
    assert (two.rows_present == one.rows_present).all() and (two.flips == one.flips).all()
    assert np.abs(two.drop_delta_sum - one.drop_delta_sum).max() <= ref.tol_totals(np.abs(dd[ok]).sum(), 40)
    sub = ref.totals_add(ref.new_totals(4), dd, kg, r.flip, r.present, rows=np.array([3, 3, -1, 40, 9]))
    assert sub.rows_present.max() <= 3


def test_case_table_inputs_are_decidable_and_routes_cover_both_sides():
    """every shape of the GPU test has a gap of 1e-3 between any two logits that an argmax compares, in the reference itself;
    and the table holds both sides of every boundary the work split has"""
    routes = []
    for i, sh in enumerate(ref.shape_table()):
        routes.append(ref.route(**sh))
        if sh["S"] * sh["W"] * sh["H"] * sh["C"] > 400_000:
            continue                                        # (the GPU test checks the large ones itself)
        case = ref.make_case(seed=100 + i, **sh)
        if sh["S"] and sh["C"] > 1:
            assert ref.min_gap(ref.run(case)) >= 1e-3, sh
    assert {r[0] for r in routes} == {ref.ROUTE_NONE, ref.ROUTE_ROW, ref.ROUTE_CHUNKED}
    assert {r[1] for r in routes} == {8, 16, 64}
    tiled = [sh for sh, r in zip(ref.shape_table(), routes) if r[3] < sh["H"]]
    assert len(tiled) >= 3 and any(r[3] == sh["H"] and sh["H"] == 128 for sh, r in zip(ref.shape_table(), routes))
