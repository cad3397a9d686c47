"""Gradients at the per-path interface on the GPU (path_grad=True: pn_pagg_backward_paths / pn_pagg_train_step_paths) against
fp64 autograd through tests/path_grads_ref.py: d loss / d path_weights on every route, and losses over encode()'s path_weight
and path_state.  Shapes, weights and bounds are those of tests/test_gpu_path_weights.py: group 0 has no live path, group 1
exactly one; every gradient, the weights' included, is held to gradcheck's bound as one more named tensor.  (Measured: the
weight gradient's largest error is 3.9e-6 of the tensor's largest element over test 1's cases and routes, against the 3e-5
allowed: profiles/path_grads.txt.)"""
import numpy as np
import pytest
import torch

import path_grads_ref as pgr
import weighted_pool_ref as wref
from gradcheck import assert_grads_close, named_grads
from test_gpu_encode import args, make
from test_gpu_pagg import TOL_OUT, zero_ok
from test_gpu_path_weights import C, F, L, N, NORMS, S, VARIANTS, WH, case

pytestmark = pytest.mark.gpu


def names_of(m):
    return [k for k, _ in m.named_parameters()]


def module(variant, H, seed, det=None):
    m = make(variant, F, H, C, L, N, seed=seed).train()
    m.set_dropout(0.0)
    m.deterministic = det
    return m


def collect(m, Xd, w=None):
    extra = {"X": Xd.grad}
    if w is not None:
        assert w.grad is not None and w.grad.shape == w.shape and w.grad.dtype == w.dtype and w.grad.device == w.device
        extra["path_weights"] = w.grad.detach().reshape(S, -1)
    return {k: v.detach().clone() for k, v in named_grads(m, extra).items()}


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("W,H", WH)
def test_weight_gradient_matches_the_fp64_reference_on_every_route(variant, norm, W, H):
    import pathnet_amd
    mask, sel, ids, codes, gm, X, Y = case(12, W)
    m = module(variant, H, 12)
    omega = wref.to_slots(variant, gm)
    pr, Xo, om = pgr.leaves(m.state_dict(), X, omega)
    out, _, _, _ = pgr.forward(variant, pr, Xo, ids, codes, sel, W, L, om, norm, path_state=False)
    cw = torch.tensor([0.5, 2.0, 1.25])
    plain = pgr.grads(names_of(m), pr, Xo, om, torch.nn.functional.cross_entropy(out, Y))
    opts = pgr.grads(names_of(m), pr, Xo, om, torch.nn.functional.cross_entropy(out, Y, weight=cw.double(), label_smoothing=0.1))
    a = args(ids, codes, mask, W, L)

    def run(route):
        m.zero_grad(set_to_none=True)
        Xd = X.cuda().requires_grad_(True)
        # the caller's tensor in its own shape, dtype and device: fp64 [S, W] on the host, fp32 [S * W] on the device
        if route == "three calls":
            w = torch.tensor(omega, dtype=torch.float64, requires_grad=True)
        else:
            w = torch.tensor(omega.reshape(-1), dtype=torch.float32, device="cuda", requires_grad=True)
        kw = dict(path_weights=w, path_weight_norm=norm, path_grad=True)
        if route == "three calls":
            logits = m(Xd, *a, **kw)
            torch.nn.functional.cross_entropy(logits, Y.cuda()).backward()
        elif route == "fused":
            loss, logits = m.forward_loss(Xd, *a, Y, fused=True, **kw)
            loss.backward()
        else:
            fn = pathnet_amd.CrossEntropyLoss(weight=cw, label_smoothing=0.1)
            loss, logits = m.forward_loss(Xd, *a, Y, fused=True, loss=fn, **kw)
            loss.backward()
        assert (logits.detach().double().cpu() - out.detach()).abs().max().item() < TOL_OUT
        return collect(m, Xd, w)
    for route, ref in (("three calls", plain), ("fused", plain), ("fused with loss options", opts)):
        got = run(route)
        assert all(bool(torch.isfinite(g).all()) for g in got.values()), route
        gw, rw = got["path_weights"].double().cpu(), ref["path_weights"]
        print("path_grads %s %s W=%d H=%d %s: weight gradient error %.3g of %.3g" % (
            variant, norm, W, H, route, (gw - rw).abs().max().item(), rw.abs().max().item()))
        # exact zeros: the empty group and every dead entry (by slot); HOMO / PAGG under "sum" are scale invariant in a group's
        # weights, so its single live path gets exactly 0 too (group 1 is row 1 of their slots)
        assert torch.count_nonzero(gw[torch.as_tensor(omega) == 0]).item() == 0, route
        if variant != "hetero" and norm == "sum":
            assert abs(rw[1, W // 2].item()) <= 1e-12 * rw.abs().max().item() and gw[1, W // 2].item() == 0.0, route
        assert_grads_close(got, ref, zero_ok=zero_ok(variant), tag="path_grads %s %s %d %d %s" % (variant, norm, W, H, route))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("norm", NORMS)
def test_dead_entries_get_zero_and_change_no_other_bit(variant, norm):
    W, H = 40, 128
    mask, sel, ids, codes, gm, X, Y = case(17, W)
    m = module(variant, H, 17, det=True)
    a = args(ids, codes, mask, W, L)
    bad = gm.copy()
    bad[0] = np.resize([np.nan, -1.0, np.inf, -np.inf, -0.0], W)
    bad[3, 1::2] = np.resize([np.nan, -1.0, np.inf], len(bad[3, 1::2]))
    clean = np.where(np.isfinite(bad) & (bad > 0), bad, 0.0)

    def run(gmw, fused):
        m.zero_grad(set_to_none=True)
        Xd = X.cuda().requires_grad_(True)
        w = torch.tensor(wref.to_slots(variant, gmw), dtype=torch.float32, device="cuda", requires_grad=True)
        if fused:
            loss, _ = m.forward_loss(Xd, *a, Y, fused=True, path_weights=w, path_weight_norm=norm, path_grad=True)
        else:
            loss = torch.nn.functional.cross_entropy(m(Xd, *a, path_weights=w, path_weight_norm=norm, path_grad=True), Y.cuda())
        loss.backward()
        return collect(m, Xd, w)
    dead = torch.as_tensor(wref.to_slots(variant, clean) == 0)
    for fused in (False, True):
        want, got = run(clean, fused), run(bad, fused)
        for k in want:
            assert bool(torch.isfinite(got[k]).all()), (fused, k)
            assert torch.equal(got[k], want[k]), (fused, k)
        assert torch.count_nonzero(got["path_weights"].cpu()[dead]).item() == 0
        assert torch.count_nonzero(got["path_weights"].cpu()[~dead]).item() > 0


def _encode_losses(enc, logits_loss, A, B, Cst):
    return {"all": logits_loss + (A * enc[1]).sum() + (B * enc[2]).sum() + (Cst * enc[3]).sum(),
            "path_weight": (B * enc[2]).sum(), "path_state": (Cst * enc[3]).sum()}


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("W,H", WH)
def test_losses_over_encode_outputs_match_the_fp64_reference(variant, weighted, W, H):
    mask, sel, ids, codes, gm, X, Y = case(21, W)
    m = module(variant, H, 21)
    omega = wref.to_slots(variant, gm) if weighted else None
    rng = np.random.default_rng(22)
    A, B, Cst = (torch.as_tensor(rng.normal(size=s)) for s in ((S, 2 * H), (S, W), (S, W, H)))
    pr, Xo, om = pgr.leaves(m.state_dict(), X, omega)
    ref_enc = pgr.forward(variant, pr, Xo, ids, codes, sel, W, L, om, "sum")
    ref_loss = _encode_losses(ref_enc, torch.nn.functional.cross_entropy(ref_enc[0], Y), A, B, Cst)
    a = args(ids, codes, mask, W, L)
    Ad, Bd, Cd = (t.float().cuda() for t in (A, B, Cst))
    for which in ("all", "path_weight", "path_state"):
        m.zero_grad(set_to_none=True)
        Xd = X.cuda().requires_grad_(True)
        w = torch.tensor(omega, dtype=torch.float32, device="cuda", requires_grad=True) if weighted else None
        enc = m.encode(Xd, *a, path_state=True, path_weights=w, path_grad=True)
        for got_t, ref_t in zip(enc, ref_enc):
            assert (got_t.detach().double().cpu() - ref_t.detach()).abs().max().item() < TOL_OUT * max(1.0, ref_t.abs().max().item())
        loss = _encode_losses(enc, torch.nn.functional.cross_entropy(enc.logits, Y.cuda()), Ad, Bd, Cd)[which]
        loss.backward()
        got = collect(m, Xd, w)
        ref = pgr.grads(names_of(m), pr, Xo, om, ref_loss[which])
        tag = "path_grads encode %s %s %d %d %s" % (variant, "weighted" if weighted else "plain", W, H, which)
        if which == "path_weight" and variant == "pagg" and not weighted:
            # the coefficients are the constant 1: exact zeros everywhere, in the reference and here
            for k in ref:
                assert torch.count_nonzero(ref[k]).item() == 0 and torch.count_nonzero(got[k]).item() == 0, k
            assert_grads_close(got, ref, zero_ok=tuple(ref), tag=tag)
            continue
        if which == "path_state" and weighted:      # the states do not depend on the weights
            assert torch.count_nonzero(got["path_weights"]).item() == 0
        if which == "path_weight" and variant == "hetero":
            # d loss / d attw.bias = sum_{s,m} coef (B - T_s / kappa_s) slope is a sum that cancels to nothing (the softmax
            # ignores a constant added to its scores), but here its TERMS are of the size of B, hundreds of times the largest
            # gradient of the case, which is what gradcheck's noise term is scaled by.  Its own bound, from the fp32 arithmetic of
            # the sum: every term carries four roundings (coef, the difference, two products) and T's own error, and the
            # W / 4 + 4 + S additions behind it one each, of at most sum |coef| (|B| + |T / kappa|) altogether
            coef = ref_enc[2].detach()
            Tk = (coef * B).sum(1, keepdim=True) / coef.sum(1, keepdim=True).clamp(min=1e-300) * (coef.sum(1, keepdim=True) > 0)
            bound = (4 + W / 4 + 4 + S) * 2.0 ** -23 * (coef.abs() * (B.abs() + Tk.abs())).sum().item()
            err = abs(got.pop("attw.bias").item() - ref.pop("attw.bias").item())
            print("%s: attw.bias error %.3g, bound %.3g" % (tag, err, bound))
            assert err <= bound
        assert_grads_close(got, ref, zero_ok=zero_ok(variant), tag=tag)


@pytest.mark.parametrize("variant", VARIANTS)
def test_micro_batches_and_slices_stay_within_the_bound_of_the_one_batch_run(variant):
    from pathnet_amd import modules
    W, H = 40, 128
    mask, sel, ids, codes, gm, X, Y = case(14, W)
    m = module(variant, H, 14)
    omega = wref.to_slots(variant, gm)
    a = args(ids, codes, mask, W, L)
    rng = np.random.default_rng(23)
    Bd, Cd = (torch.as_tensor(rng.normal(size=s), dtype=torch.float32).cuda() for s in ((S, W), (S, W, H)))
    Yd = Y.cuda()

    def run(how, slices=(None,)):
        m.zero_grad(set_to_none=True)
        Xd = X.cuda().requires_grad_(True)
        w = torch.tensor(omega, dtype=torch.float32, device="cuda", requires_grad=True)
        kw = dict(path_weights=w, path_grad=True)
        if how == "fused":
            loss, _ = m.forward_loss(Xd, *a, Y, fused=True, **kw)
        elif how == "logits":
            parts = [m(Xd, *a, group_slice=sl, **kw) for sl in slices]
            loss = torch.nn.functional.cross_entropy(torch.cat(parts), Yd)
        else:
            parts = [m.encode(Xd, *a, path_state=True, group_slice=sl, **kw) for sl in slices]
            cat = [torch.cat([p[i] for p in parts]) for i in range(4)]
            loss = torch.nn.functional.cross_entropy(cat[0], Yd) + (Bd * cat[2]).sum() + (Cd * cat[3]).sum()
        loss.backward()
        return collect(m, Xd, w)
    one = {how: run(how) for how in ("fused", "logits", "encode")}
    cut = ((0, 2), (2, 3))
    for how in ("logits", "encode"):
        assert_grads_close(run(how, cut), one[how], zero_ok=zero_ok(variant), tag="path_grads slices %s %s" % (variant, how))
    kw = dict(cell=m._cell_kind, deterministic=modules.deterministic_default(), compact=modules.compact_default())
    m.workspace_budget = modules.workspace_bytes(variant, N, F, H, C, S, W, L, batch_groups=2, **kw)
    bg = modules.pick_batch_groups(variant, N, F, H, C, S, W, L, m.workspace_budget, **kw)
    assert 0 < bg < S, bg
    for how in ("fused", "logits", "encode"):
        assert_grads_close(run(how), one[how], zero_ok=zero_ok(variant), tag="path_grads micro-batches %s %s" % (variant, how))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("W,H", WH)
def test_bits(variant, W, H):
    mask, sel, ids, codes, gm, X, Y = case(15, W)
    m = module(variant, H, 15)
    a = args(ids, codes, mask, W, L)
    omega = wref.to_slots(variant, gm)

    def run(fused, path_grad=True, leaf=True):
        m.zero_grad(set_to_none=True)
        Xd = X.cuda().requires_grad_(True)
        w = torch.tensor(omega, dtype=torch.float32, device="cuda", requires_grad=leaf)
        kw = dict(path_weights=w, path_grad=path_grad)
        if fused:
            loss, logits = m.forward_loss(Xd, *a, Y, fused=True, **kw)
        else:
            logits = m(Xd, *a, **kw)
            loss = torch.nn.functional.cross_entropy(logits, Y.cuda())
        loss.backward()
        g = collect(m, Xd, w if leaf else None)
        g["logits"] = logits.detach().clone()
        return g
    for fused in (False, True):
        # the default mode: the weight gradient is plain stores over fixed-order sums, the same bits in every run
        m.deterministic = False
        r1, r2 = run(fused), run(fused)
        assert torch.equal(r1["path_weights"], r2["path_weights"]), fused
        # the deterministic mode: every gradient
        m.deterministic = True
        r1, r2 = run(fused), run(fused)
        for k in r1:
            assert torch.equal(r1[k], r2[k]), (fused, k)
        # the keyword alone -- weights that ask for no gradient, no per-path upstream -- changes no bit
        off, on = run(fused, path_grad=False, leaf=False), run(fused, path_grad=True, leaf=False)
        for k in off:
            assert torch.equal(on[k], off[k]), (fused, k)
            assert torch.equal(r1[k], off[k]), (fused, k)      # and neither does asking for the weights' gradient


def test_gradient_descent_on_the_log_weights_lowers_the_loss():
    variant, W, H = "homo", 40, 128
    mask, sel, ids, codes, gm, X, Y = case(19, W)
    m = module(variant, H, 19, det=True)
    a = args(ids, codes, mask, W, L)
    Xd, Yd = X.cuda(), Y.cuda()
    logw = torch.zeros(S, W, device="cuda", requires_grad=True)
    losses = []
    for _ in range(11):
        loss = torch.nn.functional.cross_entropy(m(Xd, *a, path_weights=logw.exp(), path_weight_norm="count", path_grad=True), Yd)
        losses.append(loss.item())
        g, = torch.autograd.grad(loss, logw)
        assert bool(torch.isfinite(g).all()) and torch.count_nonzero(g).item() > 0
        with torch.no_grad():
            logw -= 0.5 * g
    print("path_grads descent: %.6f -> %.6f" % (losses[0], losses[-1]))
    assert losses[-1] < losses[0]


def test_refusals_and_no_grad():
    variant, W, H = "pagg", 3, 32
    mask, sel, ids, codes, gm, X, Y = case(20, W)
    m = module(variant, H, 20)
    a = args(ids, codes, mask, W, L)
    w = torch.tensor(wref.to_slots(variant, gm), dtype=torch.float32, requires_grad=True)
    with pytest.raises(ValueError, match="requires grad.*path_grad"):
        m(X.cuda(), *a, path_weights=w)
    with torch.no_grad():       # the keyword changes nothing
        off = m(X.cuda(), *a, path_weights=w.detach())
        on = m(X.cuda(), *a, path_weights=w, path_grad=True)
        enc = m.encode(X.cuda(), *a, path_state=True, path_weights=w, path_grad=True)
    assert torch.equal(on, off) and not on.requires_grad and not enc.path_state.requires_grad
    enc = m.encode(X.cuda(), *a, path_state=True)
    assert not enc.path_weight.requires_grad and not enc.path_state.requires_grad      # (without the keyword: as before)
    enc = m.encode(X.cuda(), *a, path_state=True, path_grad=True)
    assert enc.path_weight.requires_grad and enc.path_state.requires_grad
