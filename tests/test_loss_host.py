"""CPU checks of the loss options' reference (tests/loss_ref.py): it IS torch.nn.functional.cross_entropy in float64 over
class counts x weights x ignore values x smoothing x reductions, it carries the library's two stated differences from
torch, and the Python side (optim.balanced_class_weight, CrossEntropyLoss's argument handling) is right.  No GPU."""
import math

import loss_ref as R
import pytest
import torch

ROWS = 41


def _torch64(x, t, w, ii, eps, reduction):
    x64 = x.double().clone().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(x64, t, weight=None if w is None else w.double(),
                                             ignore_index=ii if ii is not None else -(10 ** 6),
                                             label_smoothing=R.f32(eps), reduction=reduction)
    loss.backward()
    return float(loss.item()), x64.grad


@pytest.mark.parametrize("reduction", R.HOST_REDUCTIONS)
@pytest.mark.parametrize("C", R.HOST_CLASSES)
def test_reference_is_torch_in_float64(C, reduction):
    """loss to 1e-12 relative, gradient to 1e-8 relative (torch takes the smoothing through a float)"""
    checked = degenerate = 0
    for weights, ignore, eps in R.host_cases():
        x, t, w, ii = R.make_case(ROWS, C, weights, ignore, seed=3)
        ref = R.loss_ref(x, t, w, ii, eps, reduction, yardstick=False)
        want, gwant = _torch64(x, t, w, ii, eps, reduction)
        if reduction == "mean" and ref["D"] == 0.0:     # (C = 1 with its one class ignored or weightless)
            assert math.isnan(ref["loss"]) and math.isnan(want), (weights, ignore, eps)
            degenerate += 1
            continue
        assert abs(ref["loss"] - want) <= 1e-12 * max(1.0, abs(want)), (weights, ignore, eps, ref["loss"], want)
        gerr = (ref["grad"] - gwant).abs().max().item()
        assert gerr <= 1e-8 * max(gwant.abs().max().item(), 1e-300), (weights, ignore, eps, gerr)
        if ii is not None:
            assert (ref["grad"][t == ii] == 0).all()
        checked += 1
    assert checked + degenerate == len(R.HOST_WEIGHTS) * len(R.HOST_IGNORE) * len(R.HOST_SMOOTHING)
    assert checked >= (12 if C == 1 else 30)


def test_fp32_yardstick_and_bounds_come_with_the_reference():
    x, t, w, ii = R.make_case(ROWS, 7, "zero", -1, seed=1)
    ref = R.loss_ref(x, t, w, ii, 0.1, "mean", grad_scale=3.0)
    lb, gb = R.loss_bounds(ref)
    assert abs(ref["loss32"] - ref["loss"]) <= lb / 8.0 + 1e-300 and lb >= 2e-6
    assert gb >= 2e-6 * ref["grad"].abs().max().item() > 0
    plain = R.loss_ref(x, t, w, ii, 0.1, "mean")
    assert abs(ref["loss"] - 3.0 * plain["loss"]) <= 1e-12 * abs(ref["loss"])


def test_reference_carries_the_two_differences_from_torch():
    x, t, w, _ = R.make_case(ROWS, 7, "random", "none", seed=2)
    base = R.loss_ref(x, t, w, -1, 0.1, "mean")
    # 1. a target outside [0, C) that is not the ignore value: NaN loss, a zero row, nothing into D, the other rows as they were
    t_bad = t.clone()
    t_bad[5] = 7
    t_bad[9] = -3
    got = R.loss_ref(x, t_bad, w, -1, 0.1, "mean")
    assert math.isnan(got["loss"]) and got["loss32"] is None
    assert (got["grad"][5] == 0).all() and (got["grad"][9] == 0).all()
    good = torch.ones(ROWS, dtype=torch.bool)
    good[5] = good[9] = False
    sub = R.loss_ref(x[good], t[good], w, -1, 0.1, "mean")
    assert got["D"] == pytest.approx(sub["D"], rel=1e-15)
    assert torch.allclose(got["grad"][good], sub["grad"], rtol=1e-13, atol=0)
    assert not torch.equal(got["grad"][good], base["grad"][good])       # (D changed: the rows are scaled differently)
    # 2. D == 0 under the mean: NaN loss and ZERO gradients -- every row ignored, or only zero-weight classes present
    all_ign = R.loss_ref(x, torch.full_like(t, -1), w, -1, 0.1, "mean", yardstick=False)
    assert math.isnan(all_ign["loss"]) and all_ign["D"] == 0.0 and (all_ign["grad"] == 0).all()
    w0 = w.clone()
    w0[2] = 0.0
    zero_w = R.loss_ref(x, torch.full_like(t, 2), w0, None, 0.0, "mean", yardstick=False)
    assert math.isnan(zero_w["loss"]) and zero_w["D"] == 0.0 and (zero_w["grad"] == 0).all()
    # (the sum has no denominator: all rows ignored is a plain zero)
    s = R.loss_ref(x, torch.full_like(t, -1), w, -1, 0.1, "sum", yardstick=False)
    assert s["loss"] == 0.0 and (s["grad"] == 0).all()
    # an ignored row's logits are not looked at
    xn = x.clone()
    xn[t == 3] = float("nan")
    a = R.loss_ref(xn, t, w, 3, 0.1, "mean", yardstick=False)
    b = R.loss_ref(x, t, w, 3, 0.1, "mean", yardstick=False)
    assert a["loss"] == b["loss"] and torch.equal(a["grad"], b["grad"])


def test_given_denominator_scales_loss_and_gradients():
    x, t, w, ii = R.make_case(ROWS, 7, "random", -100, seed=4)
    own = R.loss_ref(x, t, w, ii, 0.1, "mean")
    given = R.loss_ref(x, t, w, ii, 0.1, "mean", denominator=2.0 * own["D"])
    assert given["loss"] == pytest.approx(own["loss"] / 2.0, rel=1e-15)
    assert torch.allclose(given["grad"], own["grad"] / 2.0, rtol=1e-14, atol=0)


def test_case_tables_cover_what_the_issue_lists():
    assert set(R.HOST_CLASSES) == {1, 2, 7, 65} and set(R.HOST_SMOOTHING) == {0.0, 0.1, 1.0}
    assert set(R.HOST_IGNORE) == {"none", -100, -1, "class"} and set(R.HOST_REDUCTIONS) == {"mean", "sum"}
    assert set(R.GPU_ROWS) == {1, 63, 65, 1025, 32768, 32769} and set(R.GPU_CLASSES) == {1, 2, 65, 300}
    cols = list(zip(*R.GPU_OPTIONS.values()))
    assert {"random", "zero"} <= set(cols[0]) and {-1, -100, "class"} <= set(cols[1])
    assert {0.1, 1.0} <= set(cols[2]) and {"mean", "sum"} == set(cols[3])
    _, t, w, ii = R.make_case(33, 65, "zero", -1)
    assert (t == -1).any() and (t >= 0).any() and (w == 0).sum() == 1 and ii == -1


def test_balanced_class_weight_against_a_hand_worked_case():
    from pathnet_amd import optim
    # classes 0..3; kept rows: 0, 0, 0, 1, 2, 2 (n = 6); class 3 never occurs; -1 is ignored, 9 is no class
    t = torch.tensor([0, -1, 0, 1, 2, 9, 0, 2, -1])
    w = optim.balanced_class_weight(t, 4, ignore_index=-1)
    assert w.dtype == torch.float32 and w.shape == (4,)
    assert torch.allclose(w, torch.tensor([6 / (4 * 3), 6 / (4 * 1), 6 / (4 * 2), 0.0]), rtol=1e-6, atol=0)
    # a valid class as the ignore value: its rows do not count and its weight is 0
    w2 = optim.balanced_class_weight(torch.tensor([0, 1, 1, 2, 2, 2]), 3, ignore_index=2)
    assert torch.allclose(w2, torch.tensor([3 / (3 * 1), 3 / (3 * 2), 0.0]), rtol=1e-6, atol=0)
    # without an ignore value the -1 rows are simply no class
    w3 = optim.balanced_class_weight(torch.tensor([0, -1, 1, 1]), 2)
    assert torch.allclose(w3, torch.tensor([3 / 2, 3 / 4]), rtol=1e-6, atol=0)


def test_cross_entropy_loss_arguments():
    from pathnet_amd import _lib, optim
    bare = optim.CrossEntropyLoss()
    assert not bare.has_options and bare.ignore_index is None and list(bare.state_dict()) == []
    assert optim.CrossEntropyLoss(ignore_index=-100).has_options
    assert optim.CrossEntropyLoss(label_smoothing=0.1).has_options
    assert optim.CrossEntropyLoss(weight=[1.0, 2.0]).has_options
    assert optim.CrossEntropyLoss(reduction="sum").has_options
    with pytest.raises(ValueError):
        optim.CrossEntropyLoss(reduction="none")
    with pytest.raises(ValueError):
        optim.CrossEntropyLoss(label_smoothing=1.5)
    # the struct the library reads: field order and sizes of pn_loss_spec
    names = [f for f, _ in _lib.LossSpec._fields_]
    assert names == ["weight", "ignore_index", "has_ignore", "label_smoothing", "reduction", "grad_scale", "denominator",
                     "denominator_given"]
    assert (_lib.LOSS_MEAN, _lib.LOSS_SUM) == (0, 1)
    for name in ("pn_loss_denominator", "pn_cross_entropy_ex", "pn_pagg_train_step_loss"):
        assert hasattr(_lib.load(), name)
    assert _lib.load().pn_abi_version() == 12


def test_loss_spec_argument_errors_come_before_any_launch():
    """PN_ERR_ARG without a device: a null spec, smoothing outside [0, 1], an unknown reduction, the mean without a
    denominator -- checked ahead of every pointer and of the first launch (this test runs without a GPU)."""
    import ctypes

    from pathnet_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)       # (never dereferenced: the checks fail first)

    def spec(eps=0.0, reduction=_lib.LOSS_MEAN, denom=one):
        return _lib.LossSpec(None, 0, 0, eps, reduction, 1.0, denom, 0)
    bad = [spec(eps=-0.1), spec(eps=1.5), spec(eps=float("nan")), spec(reduction=2), spec(reduction=-1), spec(denom=None)]
    for s in bad:
        assert lib.pn_cross_entropy_ex(one, one, 4, 3, ctypes.byref(s), one, None, None) == _lib.PN_ERR_ARG
        assert lib.pn_loss_denominator(one, 4, 3, ctypes.byref(s), None) == _lib.PN_ERR_ARG
        assert lib.pn_pagg_train_step_loss(None, None, None, ctypes.byref(s), one, one, None) == _lib.PN_ERR_ARG
    assert lib.pn_cross_entropy_ex(one, one, 4, 3, None, one, None, None) == _lib.PN_ERR_ARG
    assert lib.pn_loss_denominator(one, 4, 3, None, None) == _lib.PN_ERR_ARG
    assert lib.pn_pagg_train_step_loss(None, None, None, None, one, one, None) == _lib.PN_ERR_ARG
    assert b"loss spec" in lib.pn_last_error()
    ok_sum = spec(reduction=_lib.LOSS_SUM, denom=None)          # the sum needs no denominator: the NEXT check speaks
    assert lib.pn_cross_entropy_ex(None, one, 4, 3, ctypes.byref(ok_sum), one, None, None) == _lib.PN_ERR_ARG
    assert b"null argument" in lib.pn_last_error()
