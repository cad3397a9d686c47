"""model.explain(): the public interface over pn_explain_groups, against the fp64 reference of the weighted pooling
(tests/weighted_pool_ref.py) on the module's own parameters and against the module's explicit forward(path_weights=...) calls.

Tolerance of a logit row: 1e-5 * max(1, rho).  1e-5 is what tests/test_gpu_path_weights.py holds the weighted forward to; rho
is the case's renormalisation factor as the reference reports it -- the largest ratio of a remaining member's applied
coefficient with and without the leave-out -- which multiplies the partial pooled sum and hence its fp32 error.  The inputs
keep rho <= W for every drop and for the keeps of PathNet_homo / PAGG (asserted).  PathNet's keep of a single slot has
rho = W / a_g > W by construction (its softmax weight a_g becomes 1); it is held to the same cap of 1e-5 * W, which is the
tighter reading.  The largest error seen is printed per case ("explain-error ...").
"""
import functools

import numpy as np
import pytest
import torch

import explain_ref as ref
import weighted_pool_ref as wref
from test_gpu_encode import args, case, make
from test_gpu_path_weights import reference

pytestmark = pytest.mark.gpu

N, F, S, W, L, C = 30, 12, 6, 5, 4, 3
VARIANTS = ["hetero", "homo", "pagg"]
HS = [32, 20]                   # 20: padded to 32 inside
TOL = 1e-5


@functools.lru_cache(None)
def setup(variant, H, seed=3):
    """-> (model in eval mode, X on the GPU, mask, sel, ids, codes); shared, never written to"""
    rng = np.random.default_rng(seed)
    mask, sel, ids, codes = case(rng, N, S, W, L)
    X = torch.as_tensor(rng.uniform(0, 1, (N, F)), dtype=torch.float32)
    m = make(variant, F, H, C, L, N, seed=seed).eval()
    with torch.no_grad():
        m.fc2.weight.mul_(3.0)          # logits of order one
    return m, X.cuda(), mask, sel, ids, codes


def call(variant, H, **kw):
    m, X, mask, sel, ids, codes = setup(variant, H)
    return m.explain(X, *args(ids, codes, mask, W, L), **kw)


def ratio(new, base):
    """rho as the reference reports it: the largest ratio of an applied coefficient after / before, over the members kept"""
    new, base = new.detach().numpy(), base.detach().numpy()
    kept = new != 0
    return float((new[kept] / base[kept]).max()) if kept.any() else 1.0


def leave_out_cases(variant, gm, group, G):
    """(name, g, member-order weights) of every drop and keep"""
    for g in range(G):
        R = group == g
        yield "drop_logits", g, np.where(R, 0.0, gm)
        yield "keep_logits", g, np.where(R, gm, 0.0)


def check_against_reference(variant, H, gm, norm, tag):
    m, X, mask, sel, ids, codes = setup(variant, H)
    base = np.ones((S, W)) if gm is None else gm
    pw = None if gm is None else wref.to_slots(variant, gm)
    ex = m.explain(X, *args(ids, codes, mask, W, L), groups="path", logits=True, path_weights=pw, path_weight_norm=norm)
    out0, _, coef0, _, _ = reference(variant, m, X, ids, codes, sel, W, wref.to_slots(variant, base), norm)
    assert (ex.logits.double().cpu() - out0.detach()).abs().max().item() < TOL
    group = np.tile(np.arange(W), (S, 1))
    worst = 0.0
    for name, g, omega in leave_out_cases(variant, base, group, W):
        slots = wref.to_slots(variant, omega)
        want, _, coef, _, _ = reference(variant, m, X, ids, codes, sel, W, slots, norm)
        rho = ratio(coef, coef0)
        if name == "drop_logits" or variant != "hetero":
            assert rho <= W * (1 + 1e-9), (name, g, rho)
        tol = TOL * max(1.0, min(rho, W))
        got = getattr(ex, name)[:, g].double().cpu()
        e_ref = (got - want.detach()).abs().max().item()
        with torch.no_grad():
            own = m(X, *args(ids, codes, mask, W, L), path_weights=slots, path_weight_norm=norm)
        e_own = (got - own.double().cpu()).abs().max().item()
        worst = max(worst, e_ref / tol, e_own / tol)
        assert e_ref < tol and e_own < tol, (name, g, rho, e_ref, e_own)
    print("explain-error %s H=%d %s %s: worst error / tolerance %.3g" % (variant, H, norm, tag, worst))
    live = wref.live(base).numpy() > 0
    assert (ex.present.cpu().numpy() == live.astype(np.int32)).all()
    return ex


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_path_groups_are_the_reference_and_the_modules_own_weighted_forward(variant, H):
    ex = check_against_reference(variant, H, None, "sum", "unweighted")
    assert ex.drop_logits.shape == (S, W, C) and ex.keep_logits.shape == (S, W, C) and ex.contribution is None
    assert (ex.target == ex.logits.argmax(1)).all()


@pytest.mark.parametrize("norm", ["sum", "count"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_caller_weights_with_a_dead_member(variant, norm):
    """path_weights by sequence slot, as forward() takes them; for PathNet explain re-orders them to member order"""
    rng = np.random.default_rng(5)
    gm = rng.choice([0.75, 1.0, 1.25], (S, W))         # (close to one another: rho stays below W)
    gm[:, 2] = 0.0
    gm[1, 0] = 0.0
    ex = check_against_reference(variant, 32, gm, norm, "weighted")
    assert (ex.present[:, 2] == 0).all() and (ex.flip[:, 2] == 0).all() and (ex.drop_delta[:, 2] == 0).all()


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_contributions_add_up_to_the_logits(variant, H):
    m, X, mask, sel, ids, codes = setup(variant, H)
    ex = call(variant, H, contribution=True)
    with torch.no_grad():
        enc = m.encode(X, *args(ids, codes, mask, W, L))
    # (explain's forward runs without the PN_EVAL_ZW shortcut: encode()'s logits to the forward's tolerance, not to the bit)
    assert (enc.logits - ex.logits).abs().max().item() < TOL and ex.contribution.shape == (S, W, C) and ex.drop_logits is None
    e = m.fc2.bias.double().cpu() + enc.embedding[:, :H].double().cpu() @ m.fc2.weight[:, :H].double().cpu().t()
    total = e + ex.contribution.double().cpu().sum(1)
    assert (total - ex.logits.double().cpu()).abs().max().item() < TOL


@pytest.mark.parametrize("variant", ["homo", "pagg"])
def test_reach_groups_are_the_code_maxima(variant):
    m, X, mask, sel, ids, codes = setup(variant, 32)
    by_name = call(variant, 32, groups="reach", logits=True)
    explicit = call(variant, 32, groups=torch.as_tensor(codes.max(-1)), num_groups=L, logits=True)
    inferred = call(variant, 32, groups=torch.as_tensor(codes.max(-1)))
    assert by_name.drop_delta.shape == (S, L) and inferred.drop_delta.shape[1] == int(codes.max()) + 1
    for k in ("drop_delta", "keep_gain", "flip", "present", "drop_logits", "keep_logits"):
        assert torch.equal(getattr(by_name, k), getattr(explicit, k)), k
    want = np.stack([(codes.max(-1) == g).sum(1) for g in range(L)], 1)
    assert (by_name.present.cpu().numpy() == want).all()


def test_reach_raises_on_pathnet():
    with pytest.raises(ValueError, match="reach"):
        call("hetero", 32, groups="reach")
    with pytest.raises(ValueError):
        call("homo", 32, groups="steps")
    with pytest.raises(ValueError):
        call("homo", 32, groups=torch.zeros(S, W + 1, dtype=torch.int64))


@pytest.mark.parametrize("variant", VARIANTS)
def test_batch_nodes(variant):
    """chunks of the node list give the bits of the unchunked call, for every class: a chunk of one node, and chunks that do not
    divide the six nodes (4 + 2).  (With the library's PN_EVAL_ZW shortcut on, encode()'s group_slice (0, 4) of this batch
    differs from rows 0 .. 3 of the whole-batch call by 1.3e-7 in path_state: the shortcut is taken by the slice's size.
    explain runs without it, and leaves the knob as it found it.)"""
    from pathnet_amd import _lib
    knob = _lib.get_knob("PN_EVAL_ZW")
    whole = call(variant, 32, logits=True, contribution=True)
    for step in (1, 4):
        part = call(variant, 32, logits=True, contribution=True, batch_nodes=step)
        for k in ("logits", "drop_delta", "keep_gain", "drop_logits", "keep_logits", "contribution", "flip", "present", "target"):
            assert torch.equal(getattr(whole, k), getattr(part, k)), (k, step)
        assert torch.equal(whole.totals.rows_present, part.totals.rows_present)
    assert _lib.get_knob("PN_EVAL_ZW") == knob


@pytest.mark.parametrize("variant", VARIANTS)
def test_target_given_and_default(variant):
    free = call(variant, 32, logits=True)
    assert (free.target == free.logits.argmax(1)).all()
    tgt = (free.target + 1) % C
    given = call(variant, 32, logits=True, target=tgt.cpu().numpy())
    assert (given.target == tgt).all() and torch.equal(given.drop_logits, free.drop_logits)
    lsm = lambda x: torch.log_softmax(x.double().cpu(), -1)          # noqa: E731
    for ex in (free, given):
        t = ex.target.cpu()
        lp_full = lsm(ex.logits).gather(1, t[:, None])
        lp_drop = lsm(ex.drop_logits).gather(2, t[:, None, None].expand(S, W, 1))[..., 0]
        assert (ex.drop_delta.double().cpu() - (lp_full - lp_drop)).abs().max().item() < TOL
    with pytest.raises(ValueError):
        call(variant, 32, target=np.zeros(S + 1, np.int64))


def test_totals_continue_over_two_calls_and_summary_agrees():
    m, X, mask, sel, ids, codes = setup("homo", 32)
    rng = np.random.default_rng(9)
    _, _, ids2, codes2 = case(rng, N, S, W, L)
    ids2[:, :, 0] = sel[:, None]
    first = m.explain(X, *args(ids, codes, mask, W, L), groups="reach")
    one = {k: getattr(first.totals, k).clone() for k in ref.Totals._fields}
    second = m.explain(X, *args(ids2, codes2, mask, W, L), groups="reach", totals=first.totals)
    assert second.totals is first.totals
    want = ref.new_totals(L)
    for ex in (first, second):
        ref.totals_add(want, ex.drop_delta.cpu().numpy(), ex.keep_gain.cpu().numpy(), ex.flip.cpu().numpy(),
                       ex.present.cpu().numpy())
        if ex is first:
            for k in ref.Totals._fields:
                assert (one[k].cpu().numpy() == getattr(want, k)).all(), k
    for k in ref.Totals._fields:
        assert (getattr(second.totals, k).cpu().numpy() == getattr(want, k)).all(), k
    rows = second.summary()
    assert [r["group"] for r in rows] == list(range(L))
    for g, r in enumerate(rows):
        n = int(want.rows_present[g])
        assert r["rows_present"] == n and r["members"] == int(want.members[g])
        if n:
            assert r["mean_drop_delta"] == pytest.approx(want.drop_delta_sum[g] / n, rel=1e-12, abs=1e-300)
            assert r["mean_keep_gain"] == pytest.approx(want.keep_gain_sum[g] / n, rel=1e-12, abs=1e-300)
            assert r["flip_rate"] == want.flips[g] / n
        else:
            assert r["mean_drop_delta"] == 0.0 and r["flip_rate"] == 0.0
    # summary() of a single call agrees with its own tensors
    fresh = m.explain(X, *args(ids, codes, mask, W, L), groups="path")
    pres = fresh.present.cpu().numpy() > 0
    for g, r in enumerate(fresh.summary()):
        assert r["rows_present"] == int(pres[:, g].sum())
        assert r["mean_drop_delta"] == pytest.approx(float(fresh.drop_delta.double().cpu().numpy()[:, g][pres[:, g]].mean()), rel=1e-12)
    vals, idx = fresh.top(2)
    assert vals.shape == (S, 2) and torch.equal(vals[:, 0], fresh.drop_delta.max(1).values)
    with pytest.raises(ValueError):
        m.explain(X, *args(ids, codes, mask, W, L), groups="path", totals=first.totals)      # another number of groups


@pytest.mark.parametrize("cell", ["gru", "mean"])
def test_other_cells_and_the_training_flag(cell):
    """the kernel sees final states only: every cell works; the training flag and torch's generators are left as found"""
    rng = np.random.default_rng(4)
    mask, sel, ids, codes = case(rng, N, S, W, L)
    X = torch.as_tensor(rng.uniform(0, 1, (N, F)), dtype=torch.float32).cuda()
    m = make("homo", F, 32, C, L, N, cell, seed=4).train()
    cpu_state, gpu_state = torch.get_rng_state(), torch.cuda.get_rng_state()
    ex = m.explain(X, *args(ids, codes, mask, W, L), logits=True)
    assert m.training and torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(), gpu_state)
    m.eval()
    omega = np.ones((S, W))
    omega[:, 3] = 0.0
    with torch.no_grad():
        own = m(X, *args(ids, codes, mask, W, L), path_weights=omega)
    assert (ex.drop_logits[:, 3] - own).abs().max().item() < TOL * W / (W - 1)
    m.eval()
    m.explain(X, *args(ids, codes, mask, W, L))
    assert not m.training
