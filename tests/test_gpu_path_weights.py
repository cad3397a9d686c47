"""Per-path weights in the aggregators' pooling (pn_path_weights, the pn_pagg_*_weighted entry points) and pn_path_multiplicity,
on the GPU against the fp64 reference of tests/weighted_pool_ref.py: logits within 1e-5, gradients within gradcheck's bound.

The weights of every case are drawn from {0, 0.25, 1, 3, 8}; pooling group 0 has no live path at all, group 1 exactly one.
They are made per (group, member) and handed over by sequence slot (weighted_pool_ref.to_slots: for PathNet a slot is not a
path of its row)."""
import numpy as np
import pytest
import torch

import weighted_pool_ref as wref
from gradcheck import assert_grads_close, named_grads
from test_gpu_encode import args, make
from test_gpu_pagg import TOL_OUT, zero_ok

pytestmark = pytest.mark.gpu

N, F, C, L, S = 50, 24, 3, 4, 5
VARIANTS = ["hetero", "homo", "pagg"]
NORMS = ["sum", "count"]
WH = [(3, 32), (40, 128), (70, 288)]         # fewer members than waves / the default / more than 64 lanes; 288: the HI = 16 kernels


def case(seed, W):
    rng = np.random.default_rng(seed)
    mask = np.zeros(N, bool)
    mask[rng.permutation(N)[:S]] = True
    sel = np.flatnonzero(mask)
    ids = rng.integers(0, N, (S, W, L))
    ids[:, :, 0] = sel[:, None]
    codes = np.minimum(rng.integers(0, L, (S, W, L)), np.arange(L)[None, None, :])
    gm = rng.choice([0.0, 0.25, 1.0, 3.0, 8.0], (S, W))
    gm[0] = 0.0                              # an empty group
    gm[1] = 0.0
    gm[1, W // 2] = 3.0                      # a group with a single live path
    gm[2:, 0] = 1.0                          # (the others have one at least)
    X = torch.as_tensor(rng.uniform(0, 1, (N, F)), dtype=torch.float32)
    Y = torch.as_tensor(rng.integers(0, C, S))
    return mask, sel, ids, codes, gm, X, Y


def reference(variant, m, X, ids, codes, sel, W, omega, norm, cell=None):
    pr = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    Xo = X.detach().cpu().clone().requires_grad_(True)
    out, emb, coef = wref.forward(variant, pr, Xo, ids, codes, sel, W, L, omega, norm, cell=cell)
    return out, emb, coef, pr, Xo


def ref_grads(m, pr, Xo, loss):
    for t in list(pr.values()) + [Xo]:
        t.grad = None
    loss.backward(retain_graph=True)
    ref = {k: pr[k].grad.clone() for k, _ in m.named_parameters()}
    ref["X"] = Xo.grad.clone()
    return ref


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("W", [3, 40, 70])
@pytest.mark.parametrize("H", [32, 128, 288])
def test_forward_and_encode_match_the_fp64_reference(variant, norm, W, H):
    mask, sel, ids, codes, gm, X, _ = case(11, W)
    m = make(variant, F, H, C, L, N, seed=11).eval()
    omega = wref.to_slots(variant, gm)
    out, emb, coef, _, _ = reference(variant, m, X, ids, codes, sel, W, omega, norm)
    with torch.no_grad():
        got = m(X.cuda(), *args(ids, codes, mask, W, L), path_weights=omega, path_weight_norm=norm)
        enc = m.encode(X.cuda(), *args(ids, codes, mask, W, L), path_weights=torch.as_tensor(omega).reshape(-1),
                       path_weight_norm=norm)
    assert torch.equal(enc.logits, got)
    e_out = (got.double().cpu() - out.detach()).abs().max().item()
    e_emb = (enc.embedding.double().cpu() - emb.detach()).abs().max().item()
    e_pw = (enc.path_weight.double().cpu() - coef.detach()).abs().max().item()
    print("forward %s %s W=%d H=%d: logits %.3g embedding %.3g coefficient %.3g" % (variant, norm, W, H, e_out, e_emb, e_pw))
    assert e_out < TOL_OUT and e_emb < TOL_OUT
    # the applied coefficient kappa * w * c: relative to its own size (kappa reaches W for a single live path of weight 1)
    assert e_pw < TOL_OUT * max(1.0, coef.abs().max().item())
    assert torch.count_nonzero(enc.path_weight[0]).item() == 0 and torch.count_nonzero(enc.embedding[0, H:]).item() == 0
    assert torch.count_nonzero(enc.path_weight[1]).item() == 1


def _backward_case(variant, norm, W, H, cell=None):
    import pathnet_amd
    mask, sel, ids, codes, gm, X, Y = case(12, W)
    m = make(variant, F, H, C, L, N, cell, seed=12).train()
    m.set_dropout(0.0)
    omega = wref.to_slots(variant, gm)
    out, _, _, pr, Xo = reference(variant, m, X, ids, codes, sel, W, omega, norm, cell)
    cw = torch.tensor([0.5, 2.0, 1.25])
    plain = ref_grads(m, pr, Xo, torch.nn.functional.cross_entropy(out, Y))
    opts = ref_grads(m, pr, Xo, torch.nn.functional.cross_entropy(out, Y, weight=cw.double(), label_smoothing=0.1))
    kw = dict(path_weights=omega, path_weight_norm=norm)
    a = args(ids, codes, mask, W, L)

    def run(route):
        m.zero_grad(set_to_none=True)
        Xd = X.cuda().requires_grad_(True)
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
        err = (logits.detach().double().cpu() - out.detach()).abs().max().item()
        print("backward %s %s W=%d H=%d %s: logits %.3g" % (variant, norm, W, H, route, err))
        assert err < TOL_OUT
        return named_grads(m, {"X": Xd.grad})
    for route, ref in (("three calls", plain), ("fused", plain), ("fused with loss options", opts)):
        got = run(route)
        assert all(bool(torch.isfinite(g).all()) for g in got.values()), route
        assert_grads_close(got, ref, zero_ok=zero_ok(variant), tag="path_weights %s %s %d %d %s" % (variant, norm, W, H, route))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("W,H", WH)
def test_gradients_match_the_fp64_reference_on_every_route(variant, norm, W, H):
    _backward_case(variant, norm, W, H)


@pytest.mark.parametrize("variant,cell", [("homo", "gru"), ("pagg", "mean")])
def test_other_cells_forward_and_gradients(variant, cell):
    W, H = 40, 128
    mask, sel, ids, codes, gm, X, _ = case(13, W)
    m = make(variant, F, H, C, L, N, cell, seed=13).eval()
    omega = wref.to_slots(variant, gm)
    out, _, _, _, _ = reference(variant, m, X, ids, codes, sel, W, omega, "sum", cell)
    with torch.no_grad():
        got = m(X.cuda(), *args(ids, codes, mask, W, L), path_weights=omega)
    assert (got.double().cpu() - out.detach()).abs().max().item() < TOL_OUT
    _backward_case(variant, "sum", W, H, cell)


@pytest.mark.parametrize("variant", VARIANTS)
def test_micro_batches_and_slices_give_the_one_batch_logits(variant):
    from pathnet_amd import modules
    W, H = 40, 128
    mask, sel, ids, codes, gm, X, Y = case(14, W)
    m = make(variant, F, H, C, L, N, seed=14).eval()
    omega = wref.to_slots(variant, gm)
    a = args(ids, codes, mask, W, L)
    Xd = X.cuda()
    with torch.no_grad():
        one = m(Xd, *a, path_weights=omega)
        parts = [m(Xd, *a, path_weights=omega, group_slice=(b, n)) for b, n in ((0, 2), (2, 3))]
    close = lambda x, y: (x - y).abs().max().item() < 2e-6      # noqa: E731  (the bound of the batching tests)
    assert close(torch.cat(parts), one)
    # micro-batches of two groups: the forward, and the training step's re-runs
    m.train()
    m.set_dropout(0.0)
    loss1, out1 = m.forward_loss(Xd, *a, Y, fused=True, path_weights=omega)
    assert close(out1, one)
    kw = dict(cell=m._cell_kind, deterministic=modules.deterministic_default(), compact=modules.compact_default())
    m.workspace_budget = modules.workspace_bytes(variant, N, F, H, C, S, W, L, batch_groups=2, **kw)
    bg = modules.pick_batch_groups(variant, N, F, H, C, S, W, L, m.workspace_budget, **kw)
    assert 0 < bg < S, bg
    loss2, out2 = m.forward_loss(Xd, *a, Y, path_weights=omega)
    assert close(out2, out1) and abs(loss2.item() - loss1.item()) < 2e-6
    loss2.backward()
    g2 = named_grads(m)
    m.zero_grad(set_to_none=True)
    m.workspace_budget = None
    torch.nn.functional.cross_entropy(m(Xd, *a, path_weights=omega), Y.cuda()).backward()
    assert_grads_close(g2, named_grads(m), zero_ok=zero_ok(variant))
    with torch.no_grad():
        m.eval()
        m.workspace_budget = modules.workspace_bytes(variant, N, F, H, C, S, W, L, batch_groups=2, **kw)
        assert close(m(Xd, *a, path_weights=omega), one)


def _det_grads(m, X, a, Y, fused, **kw):
    m.zero_grad(set_to_none=True)
    Xd = X.cuda().requires_grad_(True)
    if fused:
        loss, logits = m.forward_loss(Xd, *a, Y, fused=True, **kw)
    else:
        logits = m(Xd, *a, **kw)
        loss = torch.nn.functional.cross_entropy(logits, Y.cuda())
    loss.backward()
    g = {k: v.clone() for k, v in named_grads(m, {"X": Xd.grad}).items()}
    g["logits"] = logits.detach().clone()
    return g


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("W,H", WH)
def test_deterministic_mode_is_bitwise_and_all_one_weights_change_no_bit(variant, W, H):
    mask, sel, ids, codes, gm, X, Y = case(15, W)
    m = make(variant, F, H, C, L, N, seed=15).train()
    m.set_dropout(0.0)
    m.deterministic = True
    a = args(ids, codes, mask, W, L)
    omega = wref.to_slots(variant, gm)
    for fused in (False, True):
        # (1) two weighted runs: the same bits
        r1, r2 = (_det_grads(m, X, a, Y, fused, path_weights=omega) for _ in range(2))
        for k in r1:
            assert torch.equal(r1[k], r2[k]), (fused, k)
        # (2) bitwise comparison: all-one weights, either norm, against the call without weights.  Both run the same kernels in
        # this mode -- pool_fwd_kernel and pool_bwd_wg_kernel, the fused call included -- and every factor the weights add is 1.
        none = _det_grads(m, X, a, Y, fused)
        for norm in NORMS:
            ones = _det_grads(m, X, a, Y, fused, path_weights=torch.ones(S, W, dtype=torch.float64), path_weight_norm=norm)
            for k in none:
                assert torch.equal(ones[k], none[k]), (fused, norm, k)


@pytest.mark.parametrize("variant", VARIANTS)
def test_all_one_weights_on_the_default_fused_route_within_the_bounds(variant):
    """Tolerance comparison, not bitwise: without weights the fused step of this shape runs the register-resident pooling
    step, with weights the three bodies in one launch -- other summation orders, and fp32 atomics in both."""
    W, H = 40, 128
    mask, sel, ids, codes, gm, X, Y = case(16, W)
    m = make(variant, F, H, C, L, N, seed=16).train()
    m.set_dropout(0.0)
    a = args(ids, codes, mask, W, L)
    none = _det_grads(m, X, a, Y, True)
    ones = _det_grads(m, X, a, Y, True, path_weights=np.ones((S, W), np.float32))
    assert (ones.pop("logits") - none.pop("logits")).abs().max().item() < TOL_OUT
    assert_grads_close(ones, none, zero_ok=zero_ok(variant))


@pytest.mark.parametrize("variant", VARIANTS)
def test_weights_that_are_no_finite_positive_number_are_zeros(variant):
    W, H = 40, 128
    mask, sel, ids, codes, gm, X, Y = case(17, W)
    m = make(variant, F, H, C, L, N, seed=17).train()
    m.set_dropout(0.0)
    m.deterministic = True
    a = args(ids, codes, mask, W, L)
    bad = gm.copy()
    bad[0] = np.resize([np.nan, -1.0, np.inf, -np.inf, -0.0], W)
    bad[3, 1::2] = np.resize([np.nan, -3.0, np.inf], len(bad[3, 1::2]))
    clean = np.where(np.isfinite(bad) & (bad > 0), bad, 0.0)
    for fused in (False, True):
        want = _det_grads(m, X, a, Y, fused, path_weights=wref.to_slots(variant, clean))
        got = _det_grads(m, X, a, Y, fused, path_weights=wref.to_slots(variant, bad))
        for k in want:
            assert bool(torch.isfinite(got[k]).all()), (fused, k)
            assert torch.equal(got[k], want[k]), (fused, k)
    with pytest.raises(ValueError, match="negative or non-finite"):
        m(X.cuda(), *a, path_weights=wref.to_slots(variant, bad), check_weights=True)


def multiplicity_fixture():
    rng = np.random.default_rng(4)
    ids = rng.integers(0, 3, (S, 40, 2))
    codes = (ids + np.arange(S)[:, None, None]) % 2
    return ids, codes


def test_path_multiplicity_matches_numpy():
    import pathnet_amd
    ids, codes = multiplicity_fixture()
    for c in (None, codes):
        got = pathnet_amd.path_multiplicity(torch.as_tensor(ids).cuda(), None if c is None else torch.as_tensor(c).cuda())
        assert got.dtype == torch.float32 and tuple(got.shape) == (S, 40) and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), wref.path_multiplicity_np(ids, c))
        assert (got.sum(1) == 40).all()
    # codes that tell equal id sequences apart; leading axes; host input
    split = codes.copy()
    split[:, ::2, 1] = 5
    got = pathnet_amd.path_multiplicity(ids.reshape(1, S, 40, 2), split.reshape(1, S, 40, 2))
    assert np.array_equal(got.cpu().numpy()[0], wref.path_multiplicity_np(ids, split))


def test_path_multiplicity_at_and_past_the_limits():
    import pathnet_amd
    from pathnet_amd import _lib
    rng = np.random.default_rng(5)
    for W, Lw in ((512, 16), (8192, 1), (257, 3)):          # W * L = 8192 twice; more paths than threads, odd sizes
        ids = rng.integers(0, 2, (2, W, Lw))
        codes = rng.integers(0, 2, (2, W, Lw))
        got = pathnet_amd.path_multiplicity(ids, codes).cpu().numpy()
        assert np.array_equal(got, wref.path_multiplicity_np(ids, codes)), (W, Lw)
    for W, Lw in ((8193, 1), (513, 16), (2, 17)):
        with pytest.raises(_lib.PnError):
            pathnet_amd.path_multiplicity(np.zeros((1, W, Lw), np.int64))
    assert tuple(pathnet_amd.path_multiplicity(np.zeros((0, 4, 2), np.int64)).shape) == (0, 4)


@pytest.mark.parametrize("variant", ["homo", "pagg"])
def test_multiplicities_as_weights_change_nothing(variant):
    """a row's distinct paths once each, weighted by their counts (norm "sum") = the row itself.  (Not for the hetero class:
    its pooling slots are not its rows' paths.)"""
    import pathnet_amd
    H, W, Lw = 64, 40, 4
    rng = np.random.default_rng(6)
    mask = np.zeros(N, bool)
    mask[rng.permutation(N)[:S]] = True
    sel = np.flatnonzero(mask)
    # nine distinct paths per row at the most: the last two steps from {0, 1, 2}, as in the multiplicity fixture
    tail, _ = multiplicity_fixture()
    ids = np.concatenate([np.broadcast_to(sel[:, None, None], (S, W, 2)), tail + 7], axis=2)
    codes = np.concatenate([np.zeros((S, W, 1), np.int64), np.ones((S, W, 1), np.int64), (tail + np.arange(S)[:, None, None]) % 2 + 2],
                           axis=2)
    codes = np.minimum(codes, np.arange(Lw)[None, None, :])
    m = make(variant, F, H, C, Lw, N, seed=18).eval()
    X = torch.rand(N, F).cuda()
    a = args(ids, codes, mask, W, Lw)
    mult = pathnet_amd.path_multiplicity(torch.as_tensor(ids).cuda(), torch.as_tensor(codes).cuda())
    assert (mult == 0).sum().item() >= S * (W - 9)
    with torch.no_grad():
        plain = m(X, *a)
        weighted = m(X, *a, path_weights=mult)
    assert (weighted - plain).abs().max().item() < TOL_OUT


def test_train_fixed_indices_with_a_weights_callable(tmp_path):
    import pathnet_amd
    from pathnet_amd import trainer
    rng = np.random.default_rng(7)
    n, W, H, E = 40, 6, 32, 3
    X = torch.as_tensor(rng.uniform(0, 1, (n, F)), dtype=torch.float32)
    Y = torch.as_tensor(rng.integers(0, C, n))
    ids = rng.integers(0, n, (E, n, W, L))
    ids[:, :, :, 0] = np.arange(n)[None, :, None]
    codes = np.minimum(rng.integers(0, L, (E, n, W, L)), np.arange(L))
    paths = (torch.as_tensor(ids, dtype=torch.int32), torch.as_tensor(codes, dtype=torch.uint8))
    tr, va, te = np.arange(0, 20), np.arange(20, 30), np.arange(30, 40)

    def run(tag, **kw):
        torch.manual_seed(19)
        m = pathnet_amd.PathNet_homo(F, H, C, L, dropout=0.0).cuda()
        m.deterministic = True
        res = trainer.train_fixed_indices(X, Y, C, "cora", tr, va, te, W, H, L, paths, epochs=E, dropout=0.0,
                                          save_dir=str(tmp_path / tag), model=m, **kw)
        return res, {k: v.detach().clone() for k, v in m.state_dict().items()}
    seen = []

    def ones(ids_, codes_, nodes32, epoch):
        seen.append((tuple(ids_.shape), tuple(codes_.shape), int(nodes32.numel()), epoch))
        return torch.ones(ids_.shape[:2], dtype=torch.float64)
    base, sd0 = run("base")
    for tag, fn in (("none", lambda *a: None), ("ones", ones)):
        res, sd = run(tag, path_weights=fn)
        assert res == base, tag
        for k in sd0:
            assert torch.equal(sd[k], sd0[k]), (tag, k)
    assert {s[3] for s in seen} == {0, 1, 2} and all(s[0] == (s[2], W, L) == s[1] for s in seen)
    assert {s[2] for s in seen} >= {20, 10}                  # the training step and the validation forward

    def half(ids_, codes_, nodes32, epoch):
        w = torch.ones(ids_.shape[:2], device=ids_.device)
        w[:, ::2] = 0.0
        return w
    res, sd = run("half", path_weights=half)
    assert len(res) == 5 and all(np.isfinite(r) and 0.0 <= r <= 1.0 for r in res)
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())
    assert any(not torch.equal(sd[k], sd0[k]) for k in sd0)
