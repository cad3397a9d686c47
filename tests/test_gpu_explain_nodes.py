"""model.explain(groups="node" | "edge"): the public interface over pn_explain_units / pn_explain_overlap /
pn_explain_node_totals, against the fp64 reference of the weighted pooling (tests/weighted_pool_ref.py) on the module's own
parameters and against the module's explicit forward(path_weights=...) calls, with the setup of tests/test_gpu_explain.py.

Column g of row s is the row's g-th unit (a node, or an edge); its drop is the forward with the members that touch the unit at
weight 0, its keep the forward with every other member at weight 0.  Rows with fewer than g + 1 units have an empty group
there: drop = the unchanged forward, keep = the forward with every weight 0.  So one reference forward and one forward of the
module per column and kind check every row at once.

Tolerance of a logit row: test_gpu_explain.py's rule, 1e-5 * max(1, rho), rho the renormalisation factor as the reference
reports it.  Removing a node can leave PathNet one slot of small softmax weight, rho > W: that row is still held to
1e-5 * rho, and rho is printed ("explain-nodes-rho ...").  The largest error seen is printed per case.
"""
import numpy as np
import pytest
import torch

import explain_units_ref as uref
import pathnet_amd
import weighted_pool_ref as wref
from test_gpu_encode import args, case
from test_gpu_explain import C, L, N, S, TOL, VARIANTS, W, call, ratio, setup
from test_gpu_path_weights import reference

pytestmark = pytest.mark.gpu
HS = [32, 20]
KIND = {"node": uref.UNIT_NODE, "edge": uref.UNIT_EDGE}


def expected_units(variant, H, kind, exclude_self=True):
    """the restatement's (unit, count, label) of the shared setup"""
    m, X, mask, sel, ids, codes = setup(variant, H)
    node = pathnet_amd.member_nodes(variant, torch.as_tensor(ids), S, W, L).numpy()
    return uref.units(node, KIND[kind], sel if kind == "node" and exclude_self else None)


def check_units(variant, H, kind, tag, **kw):
    m, X, mask, sel, ids, codes = setup(variant, H)
    unit, count, label = expected_units(variant, H, kind, kw.get("exclude_self", True))
    G = unit.shape[1]
    ex = call(variant, H, groups=kind, logits=True, **kw)
    assert ex.unit.dtype == torch.int64 and ex.unit_count.dtype == torch.int32 and len(ex) == 10
    assert (ex.unit.cpu().numpy() == unit).all() and (ex.unit_count.cpu().numpy() == count).all()
    assert ex.drop_logits.shape == (S, G, C) and ex.drop_delta.shape == (S, G)
    touch = uref.touches(label, G)                              # [S, G, W]
    assert (ex.present.cpu().numpy() == touch.sum(2)).all()
    ones = np.ones((S, W))
    out0, _, coef0, _, _ = reference(variant, m, X, ids, codes, sel, W, wref.to_slots(variant, ones), "sum")
    assert (ex.logits.double().cpu() - out0.detach()).abs().max().item() < TOL
    worst, hubs = 0.0, 0
    for g in range(int(count.max())):
        R = touch[:, g]                                         # [S, W]; all False where the row has no g-th unit
        has = R.any(1)
        for name, omega in (("drop_logits", np.where(R, 0.0, ones)), ("keep_logits", np.where(R, ones, 0.0))):
            omega = np.where(has[:, None], omega, ones if name == "drop_logits" else 0.0)
            slots = wref.to_slots(variant, omega)
            want, _, coef, _, _ = reference(variant, m, X, ids, codes, sel, W, slots, "sum")
            with torch.no_grad():
                own = m(X, *args(ids, codes, mask, W, L), path_weights=slots, path_weight_norm="sum")
            got = getattr(ex, name)[:, g].double().cpu()
            for s in range(S):
                rho = ratio(coef[s], coef0[s])
                if rho > W * (1 + 1e-9):
                    print("explain-nodes-rho %s H=%d %s %s column %d row %d: rho %.3g" % (variant, H, kind, name, g, s, rho))
                    assert variant == "hetero", (name, g, s, rho)      # PathNet_homo / PAGG: at most W / 1
                tol = TOL * max(1.0, rho)
                e_ref = (got[s] - want[s].detach()).abs().max().item()
                e_own = (got[s] - own[s].double().cpu()).abs().max().item()
                worst = max(worst, e_ref / tol, e_own / tol)
                assert e_ref < tol and e_own < tol, (name, g, s, rho, e_ref, e_own)
        hubs += int(R.all(1).sum())
    print("explain-nodes-error %s H=%d %s %s: worst error / tolerance %.3g, %d units on every path"
          % (variant, H, kind, tag, worst, hubs))
    return ex, unit, count, label


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_node_groups_are_the_reference_and_the_modules_own_weighted_forward(variant, H):
    ex, unit, count, label = check_units(variant, H, "node", "exclude_self")
    m, X, mask, sel, ids, codes = setup(variant, H)
    assert not (unit == sel[:, None]).any()                     # the row's own node is no unit
    assert torch.equal(ex.units(), ex.unit)
    vals, keys = ex.top_units(3)
    v2, idx = ex.top(3)
    assert torch.equal(vals, v2) and torch.equal(keys, torch.gather(ex.unit, 1, idx)) and keys.shape == (S, 3)
    assert isinstance(ex.totals, pathnet_amd.NodeTotals) and ex.totals.n_nodes == N


@pytest.mark.parametrize("variant", VARIANTS)
def test_exclude_self_false_adds_exactly_the_rows_own_node_and_a_unit_on_every_path_drops_to_e(variant):
    """Without the exclusion the row's own node is a unit; in a PathNet_homo / PAGG row it sits on every path (step 0), so
    at least one unit there is on every member: its drop is the forward with every weight 0, i.e. the logits without paths."""
    m, X, mask, sel, ids, codes = setup(variant, 32)
    ex, unit, count, label = check_units(variant, 32, "node", "with the own node", exclude_self=False)
    base = call(variant, 32, groups="node", logits=True)
    bu, bc = base.unit.cpu().numpy(), base.unit_count.cpu().numpy()
    node = pathnet_amd.member_nodes(variant, torch.as_tensor(ids), S, W, L).numpy()
    for s in range(S):
        mine, theirs = unit[s, :count[s]].tolist(), bu[s, :bc[s]].tolist()
        on_path = int(sel[s]) in node[s]
        assert set(mine) - set(theirs) == ({int(sel[s])} if on_path else set()) and set(theirs) <= set(mine)
        for k in ("drop_delta", "keep_gain", "flip", "present", "drop_logits", "keep_logits"):     # the shared units: the same bits
            a, b = getattr(ex, k)[s].cpu().numpy(), getattr(base, k)[s].cpu().numpy()
            assert a[[mine.index(u) for u in theirs]].tobytes() == b[:bc[s]].tobytes(), (k, s)
    touch = uref.touches(label, unit.shape[1])
    hub = touch.all(2)                                          # [S, G]: on every member
    if variant != "hetero":
        assert (hub.sum(1) >= 1).all() and all(hub[s, unit[s].tolist().index(int(sel[s]))] for s in range(S))
    # (PathNet: the scramble spreads a node's paths over the batch's slots, and no node of this setup sits on all five slots
    #  of a row -- checked on the host; the loop below then has nothing to do for it)
    with torch.no_grad():
        none = m(X, *args(ids, codes, mask, W, L), path_weights=np.zeros((S, W)))
    for s, g in zip(*np.nonzero(hub)):
        assert (ex.drop_logits[s, g] - none[s]).abs().max().item() < TOL, (s, g)
        assert ex.present[s, g].item() == W


@pytest.mark.parametrize("variant", ["homo", "pagg"])
def test_edge_groups(variant):
    ex, unit, count, label = check_units(variant, 32, "edge", "edges")
    assert ex.totals is None and ex.unit.shape == (S, W * (L - 1))
    ends = ex.units()
    assert ends.dtype == torch.int32 and tuple(ends.shape) == (S, W * (L - 1), 2)
    want = np.where((unit >= 0)[..., None], uref.edge_ends(unit), -1)
    assert (ends.cpu().numpy() == want).all() and (want[..., 0] <= want[..., 1]).all()
    with pytest.raises(ValueError, match="no totals"):
        ex.summary()


def test_edge_raises_on_pathnet_and_the_limits_are_named():
    m, X, mask, sel, ids, codes = setup("homo", 32)
    with pytest.raises(ValueError, match="edge"):
        call("hetero", 32, groups="edge")
    with pytest.raises(ValueError, match="num_groups"):
        call("homo", 32, groups="node", num_groups=W)
    assert call("homo", 32, groups="node", num_groups=W * L).drop_delta.shape == (S, W * L)
    with pytest.raises(ValueError, match="NodeTotals"):
        call("homo", 32, groups="node", totals=call("homo", 32).totals)             # a Totals: the wrong kind
    with pytest.raises(ValueError, match="NodeTotals"):
        call("homo", 32, groups="node", totals=pathnet_amd.NodeTotals(N + 1, "cuda"))
    with pytest.raises(ValueError, match="no totals"):
        call("homo", 32, groups="edge", totals=pathnet_amd.NodeTotals(N, "cuda"))
    with pytest.raises(ValueError):
        call("homo", 32, groups="path", totals=pathnet_amd.NodeTotals(N, "cuda"))
    rng = np.random.default_rng(2)
    for W2, L2, msg in ((65, 16, "W \\* M <= 1024"), (3, 17, "L <= 16")):
        mask2, sel2, ids2, codes2 = case(rng, N, 2, W2, L2)
        with pytest.raises(ValueError, match=msg):              # (refused before anything is launched)
            m.explain(X, *args(ids2, codes2, mask2, W2, L2), groups="node")


@pytest.mark.parametrize("kind", ["node", "edge"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_batch_nodes_leaves_the_bits_of_the_whole_call(variant, kind):
    if kind == "edge" and variant == "hetero":
        with pytest.raises(ValueError):
            call(variant, 32, groups=kind, batch_nodes=4)
        return
    whole = call(variant, 32, groups=kind, logits=True, contribution=True)
    for step in (1, 4):
        part = call(variant, 32, groups=kind, logits=True, contribution=True, batch_nodes=step)
        for k in ("logits", "drop_delta", "keep_gain", "drop_logits", "keep_logits", "contribution", "flip", "present", "target",
                  "unit", "unit_count"):
            assert torch.equal(getattr(whole, k), getattr(part, k)), (k, step)
        if kind == "node":
            assert torch.equal(whole.totals.state, part.totals.state) and whole.totals.state.sum().item() > 0


def test_path_weights_and_a_target_go_through():
    """a dead member is in no unit's count; target= changes the scores, not the logits"""
    m, X, mask, sel, ids, codes = setup("homo", 32)
    gm = np.ones((S, W))
    gm[:, 2] = 0.0
    unit, count, label = expected_units("homo", 32, "node")
    ex = call("homo", 32, groups="node", logits=True, path_weights=gm)
    label = label.copy()
    label[:, 2] = -1
    assert (ex.present.cpu().numpy() == uref.touches(label, W * L).sum(2)).all()
    g = 0
    R = uref.touches(label, W * L)[:, g]
    with torch.no_grad():
        own = m(X, *args(ids, codes, mask, W, L), path_weights=np.where(R, 0.0, gm))
    assert (ex.drop_logits[:, g] - own).abs().max().item() < TOL * W
    tgt = (ex.target + 1) % C
    given = call("homo", 32, groups="node", logits=True, path_weights=gm, target=tgt.cpu().numpy())
    assert (given.target == tgt).all() and torch.equal(given.drop_logits, ex.drop_logits)
    assert not torch.equal(given.drop_delta, ex.drop_delta)


def test_node_totals_continue_over_two_calls_and_summary_agrees():
    m, X, mask, sel, ids, codes = setup("homo", 32)
    rng = np.random.default_rng(9)
    _, _, ids2, codes2 = case(rng, N, S, W, L)
    ids2[:, :, 0] = sel[:, None]
    first = m.explain(X, *args(ids, codes, mask, W, L), groups="node")
    one = first.totals.state.clone()
    second = m.explain(X, *args(ids2, codes2, mask, W, L), groups="node", totals=first.totals)
    assert second.totals is first.totals
    want = uref.new_table(N)
    for ex in (first, second):
        uref.node_totals_add(want, ex.unit.cpu().numpy(), ex.drop_delta.cpu().numpy(), ex.keep_gain.cpu().numpy(),
                             ex.flip.cpu().numpy(), ex.present.cpu().numpy())
        if ex is first:
            assert (one.cpu().numpy() == np.stack(want)).all()
    t = second.totals
    for k in uref.NodeTable._fields:
        assert (getattr(t, k).cpu().numpy() == getattr(want, k)).all(), k
    assert want.top.sum() == 2 * S and want.rows_present.sum() == first.unit_count.sum().item() + second.unit_count.sum().item()
    rows = t.summary(k=5)
    assert rows == second.summary()[:5] and len(rows) == 5
    order = sorted(np.flatnonzero(want.rows_present), key=lambda i: (-want.flips[i], i))[:5]
    assert [r["node"] for r in rows] == [int(i) for i in order]
    for r in rows:
        i = r["node"]
        assert (r["rows_present"], r["members"], r["flips"], r["top"]) == tuple(int(getattr(want, k)[i]) for k in uref.NodeTable._fields)
        assert r["flip_rate"] == want.flips[i] / want.rows_present[i]
    assert len(t.summary()) == min(20, int((want.rows_present > 0).sum()))
