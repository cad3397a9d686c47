"""Per-path weights of the pooling, the parts that need no GPU: the fp64 reference against the oracle and against itself
(integer weights = repeated paths), the NumPy statement of pn_path_multiplicity, and what the Python surface refuses."""
import numpy as np
import pytest
import torch

from oracle import pagg_oracle as po
import weighted_pool_ref as wref

N, F, H, C, L = 30, 10, 8, 3, 4


def params_for(variant, rng):
    t = lambda *s: torch.as_tensor(rng.uniform(-0.5, 0.5, s))      # noqa: E731
    p = {"fc0.weight": t(H, F), "fc0.bias": t(H), "fc2.weight": t(C, 2 * H), "fc2.bias": t(C)}
    for d in range(L):
        name = ("nei%d" % d) if variant == "pagg" else ("nets.%d" % d)
        p[name + ".weight"], p[name + ".bias"] = t(H, H), t(H)
    G, cell = (1, "RNN") if variant == "pagg" else (4, "LSTM")
    for k, s in (("weight_ih_l0", (G * H, H)), ("weight_hh_l0", (G * H, H)), ("bias_ih_l0", (G * H,)), ("bias_hh_l0", (G * H,))):
        p["%s.%s" % (cell, k)] = t(*s)
    if variant != "pagg":
        p["attw.weight"], p["attw.bias"] = t(1, 2 * H), t(1)
    return p


def paths(rng, S, W):
    sel = np.sort(rng.permutation(N)[:S])
    ids = rng.integers(0, N, (S, W, L))
    ids[:, :, 0] = sel[:, None]
    codes = np.minimum(rng.integers(0, L, (S, W, L)), np.arange(L)[None, None, :])
    return sel, ids, codes


@pytest.mark.parametrize("variant", po.VARIANTS)
@pytest.mark.parametrize("norm", ["sum", "count"])
def test_all_one_weights_are_the_oracle(variant, norm):
    rng = np.random.default_rng(1)
    S, W = 6, 5
    p, X = params_for(variant, rng), torch.as_tensor(rng.uniform(0, 1, (N, F)))
    sel, ids, codes = paths(rng, S, W)
    want, it = po.forward(variant, p, X, ids, codes, sel, W, L, dtype=torch.float64, return_intermediates=True)
    for omega in (None, np.ones((S, W))):
        out, emb, coef = wref.forward(variant, p, X, ids, codes, sel, W, L, omega, norm)
        assert (out - want).abs().max().item() < 1e-12
        assert (emb[:, H:] - it["pooled"]).abs().max().item() < 1e-12
    if variant == "hetero":
        assert (coef - it["att"].view(S, W)).abs().max().item() < 1e-12
    elif variant == "homo":
        assert (coef - (1.0 + it["att"].view(S, W))).abs().max().item() < 1e-12
    else:
        assert torch.equal(coef, torch.ones(S, W, dtype=torch.float64))


@pytest.mark.parametrize("variant", ["homo", "pagg"])
def test_integer_weights_are_repeated_paths(variant):
    """norm="sum": a row whose path m carries the integer weight w_m pools like the row with path m written w_m times"""
    rng = np.random.default_rng(2)
    S, W = 5, 4
    p, X = params_for(variant, rng), torch.as_tensor(rng.uniform(0, 1, (N, F)))
    sel, ids, codes = paths(rng, S, W)
    omega = np.stack([rng.permutation([2, 1, 0, 3]) for _ in range(S)])         # every row: 6 paths after the expansion
    rep = lambda a: np.stack([np.repeat(a[s], omega[s], axis=0) for s in range(S)])      # noqa: E731
    got, _, _ = wref.forward(variant, p, X, ids, codes, sel, W, L, omega, "sum")
    want = po.forward(variant, p, X, rep(ids), rep(codes), sel, 6, L, dtype=torch.float64)
    assert (got - want).abs().max().item() < 1e-12
    # "count" is another value: the weights are applied as given (they sum to 6, not to W = 4)
    other, _, _ = wref.forward(variant, p, X, ids, codes, sel, W, L, omega, "count")
    assert (other - want).abs().max().item() > 1e-3


@pytest.mark.parametrize("variant", po.VARIANTS)
def test_dead_weights_count_as_zero_and_an_empty_row_pools_nothing(variant):
    rng = np.random.default_rng(3)
    S, W = 4, 5
    p, X = params_for(variant, rng), torch.as_tensor(rng.uniform(0, 1, (N, F)))
    sel, ids, codes = paths(rng, S, W)
    gm = rng.choice([0.25, 1.0, 3.0], (S, W))
    gm[0] = 0.0
    bad = gm.copy()
    bad[0] = [np.nan, -1.0, np.inf, -np.inf, 0.0]
    a = wref.forward(variant, p, X, ids, codes, sel, W, L, wref.to_slots(variant, gm))
    b = wref.forward(variant, p, X, ids, codes, sel, W, L, wref.to_slots(variant, bad))
    for x, y in zip(a, b):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())
    assert torch.count_nonzero(a[1][0, H:]).item() == 0 and torch.count_nonzero(a[2][0]).item() == 0


def multiplicity_fixture(S=5):
    rng = np.random.default_rng(4)
    ids = rng.integers(0, 3, (S, 40, 2))
    codes = (ids + np.arange(S)[:, None, None]) % 2
    return ids, codes


def test_numpy_multiplicity_rows_sum_to_w():
    ids, codes = multiplicity_fixture()
    for c in (None, codes):
        mult = wref.path_multiplicity_np(ids, c)
        assert mult.shape == (5, 40) and (mult.sum(1) == 40).all()
        assert ((mult > 0).sum(1) <= 9).all()          # nine distinct paths at the most
        assert (mult[:, 0] >= 1).all()                  # the first path is always the first of its kind
    # codes that split equal id sequences give more, smaller classes
    split = codes.copy()
    split[:, ::2, 1] = 5
    assert (wref.path_multiplicity_np(ids, split) > 0).sum() > (wref.path_multiplicity_np(ids, codes) > 0).sum()


def test_as_path_weights_shapes_and_dtypes():
    from pathnet_amd import modules
    w = modules.as_path_weights(np.ones((3, 4)), 3, 4)
    assert w.dtype == torch.float32 and tuple(w.shape) == (3, 4)
    assert tuple(modules.as_path_weights(torch.ones(12, dtype=torch.float64), 3, 4).shape) == (3, 4)
    assert modules.as_path_weights(None, 3, 4) is None
    for bad in (np.ones((4, 3)), np.ones(11), np.ones((3, 4, 1)), np.ones((2, 4))):
        with pytest.raises(ValueError, match="path_weights of shape"):
            modules.as_path_weights(bad, 3, 4)
    with pytest.raises(ValueError, match="requires grad"):
        modules.as_path_weights(torch.ones(3, 4, requires_grad=True), 3, 4)
    for bad in (-1.0, float("nan"), float("inf")):
        w = torch.ones(3, 4)
        w[1, 2] = bad
        modules.as_path_weights(w, 3, 4)                # unchecked: the kernels count the entry as 0
        with pytest.raises(ValueError, match="negative or non-finite"):
            modules.as_path_weights(w, 3, 4, check=True)


@pytest.mark.parametrize("variant", po.VARIANTS)
def test_module_refuses_bad_weights_before_it_needs_a_device(variant):
    import pathnet_amd
    cls = {"hetero": pathnet_amd.PathNet, "homo": pathnet_amd.PathNet_homo, "pagg": pathnet_amd.PAGG}[variant]
    m = cls(F, 32, C, L if variant != "pagg" else N)
    rng = np.random.default_rng(5)
    S, W = 4, 3
    sel, ids, codes = paths(rng, S, W)
    mask = np.zeros(N, bool)
    mask[sel] = True
    a = (torch.rand(N, F), torch.as_tensor(ids.reshape(S, W * L)), W, L, mask, torch.as_tensor(codes))
    for call in (m.forward, m.encode, lambda *x, **k: m.forward_loss(*x, torch.zeros(S, dtype=torch.long), **k)):
        with pytest.raises(ValueError, match="path_weights of shape"):
            call(*a, path_weights=torch.ones(S, W + 1))
        with pytest.raises(ValueError, match="requires grad"):
            call(*a, path_weights=torch.ones(S, W, requires_grad=True))
        with pytest.raises(ValueError, match="path_weight_norm"):
            call(*a, path_weights=torch.ones(S, W), path_weight_norm="mean")
        with pytest.raises(ValueError, match="negative or non-finite"):
            call(*a, path_weights=-torch.ones(S, W), check_weights=True)
        with pytest.raises(TypeError):      # keyword-only: the reference's positional call cannot reach them
            m.forward(*a, None, False, None, torch.ones(S, W))
