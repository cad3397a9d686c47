"""Gradients at the per-path interface, the parts that need no GPU: the fp64 reference's weight gradient against central
differences and its exact zeros, the scale invariance of norm="sum", the C ABI's new symbols and refusals, and the opt-in of
the Python surface."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from oracle import pagg_oracle as po
from pathnet_amd import _lib
import path_grads_ref as pgr
import weighted_pool_ref as wref
from test_path_weights_cpu import C, F, L, N, params_for, paths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, W = 5, 6


def case(variant, seed):
    rng = np.random.default_rng(seed)
    p, X = params_for(variant, rng), torch.as_tensor(rng.uniform(0, 1, (N, F)))
    sel, ids, codes = paths(rng, S, W)
    gm = rng.choice([0.25, 1.0, 3.0, 8.0], (S, W))
    gm[0] = 0.0                                     # an empty group
    gm[1] = 0.0
    gm[1, W // 2] = 3.0                             # a single live path
    gm[2, :5] = [0.0, -1.0, np.nan, np.inf, -np.inf]    # dead entries next to a live one
    Y = torch.as_tensor(rng.integers(0, C, S))
    A = torch.as_tensor(rng.normal(size=(S, W)))
    return p, X, sel, ids, codes, gm, Y, A


def loss_of(variant, norm, p, X, sel, ids, codes, omega, Y, A):
    out, _, coef = wref.forward(variant, p, X, ids, codes, sel, W, L, omega, norm)
    return torch.nn.functional.cross_entropy(out, Y) + (A * coef).sum()


@pytest.mark.parametrize("variant", po.VARIANTS)
@pytest.mark.parametrize("norm", ["sum", "count"])
def test_reference_weight_gradient_matches_central_differences_and_is_zero_where_dead(variant, norm):
    p, X, sel, ids, codes, gm, Y, A = case(variant, 31)
    om = torch.as_tensor(wref.to_slots(variant, gm), dtype=torch.float64).requires_grad_(True)
    g, = torch.autograd.grad(loss_of(variant, norm, p, X, sel, ids, codes, om, Y, A), om)
    assert bool(torch.isfinite(g).all())
    dead = ~(np.isfinite(gm) & (gm > 0))
    dead[0] = True
    g_gm = g.numpy().reshape(W, S).T if variant == "hetero" else g.numpy()      # back to (group, member): to_slots' inverse
    assert np.count_nonzero(g_gm[dead]) == 0 and np.count_nonzero(g_gm[~dead]) > 0
    # central differences at every live entry
    base = om.detach().clone()
    flat = base.reshape(-1)
    live = np.flatnonzero(np.isfinite(flat.numpy()) & (flat.numpy() > 0))
    for i in live:
        h = 1e-6 * float(flat[i])
        vals = []
        for sgn in (1.0, -1.0):
            w = flat.clone()
            w[i] += sgn * h
            vals.append(loss_of(variant, norm, p, X, sel, ids, codes, w.view(S, W), Y, A).item())
        fd = (vals[0] - vals[1]) / (2 * h)
        assert abs(fd - g.reshape(-1)[i].item()) <= 1e-6 * max(1.0, abs(fd)), (i, fd, g.reshape(-1)[i].item())


@pytest.mark.parametrize("variant", ["homo", "pagg"])
def test_sum_norm_is_scale_invariant_per_group(variant):
    """HOMO / PAGG under "sum": a group's coefficients do not change when its weights are scaled, so sum_j w_j g_j = 0 --
    in particular a single live path gets exactly 0.  (Not so for HETERO: its coefficients scale with 1 / weights.)"""
    p, X, sel, ids, codes, gm, Y, A = case(variant, 32)
    om = torch.as_tensor(wref.to_slots(variant, gm), dtype=torch.float64).requires_grad_(True)
    g, = torch.autograd.grad(loss_of(variant, "sum", p, X, sel, ids, codes, om, Y, A), om)
    wg = wref.live(om.detach()) * g
    assert bool((wg.sum(1).abs() <= 1e-12 * wg.abs().sum(1)).all())
    assert g[1, W // 2].item() == 0.0


@pytest.mark.parametrize("variant", po.VARIANTS)
def test_reference_path_states_are_in_the_coefficients_member_order(variant):
    """the pooled half of the embedding is the mean of coefficient x state over the members, in the order both are returned"""
    p, X, sel, ids, codes, gm, _, _ = case(variant, 33)
    out, emb, coef, ps = pgr.forward(variant, p, X, ids, codes, sel, W, L, wref.to_slots(variant, gm), "sum")
    H = ps.shape[2]
    assert tuple(ps.shape) == (S, W, H) and tuple(coef.shape) == (S, W)
    assert ((coef.unsqueeze(-1) * ps).sum(1) / W - emb[:, H:]).abs().max().item() < 1e-12


def test_abi_is_still_12_and_the_args_tail_is_unchanged():
    names = [f[0] for f in _lib.PaggArgs._fields_]
    assert _lib.ABI_VERSION == 12 and _lib.load().pn_abi_version() == 12
    assert names[names.index("step_state") + 1:] == ["out_embed", "out_path_weight", "out_path_state", "g_embed"]
    assert [f[0] for f in _lib.PathWeights._fields_] == ["weight", "norm"]
    assert [f[0] for f in _lib.PathGrads._fields_] == ["g_path_state", "g_path_weight", "g_weight"]


def test_new_symbols_in_header_library_and_signatures():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pathnet_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("pn_pagg_backward_paths", "pn_pagg_train_step_paths"):
        proto = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
        assert proto, name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    body = txt[txt.index("typedef struct pn_path_grads"):txt.index("} pn_path_grads;")]
    assert re.findall(r"\*\s*(\w+);", body) == ["g_path_state", "g_path_weight", "g_weight"]


def test_the_entry_points_refuse_before_they_look_at_the_device():
    lib = _lib.load()
    a = _lib.PaggArgs()
    one = ctypes.c_void_p(256)
    w = _lib.PathWeights(256, _lib.PATH_NORM_SUM)
    # the training step takes g_weight only
    for k in ("g_path_state", "g_path_weight"):
        pg = _lib.PathGrads()
        setattr(pg, k, 256)
        rc = lib.pn_pagg_train_step_paths(None, ctypes.byref(a), None, None, ctypes.byref(w), ctypes.byref(pg), one, 1.0, one, None)
        assert rc == _lib.PN_ERR_ARG, k
        assert k in lib.pn_last_error().decode()
    # g_weight without the weights it is the gradient of
    pg = _lib.PathGrads(None, None, 256)
    for pw in (None, ctypes.byref(_lib.PathWeights(None, _lib.PATH_NORM_SUM))):
        assert lib.pn_pagg_train_step_paths(None, ctypes.byref(a), None, None, pw, ctypes.byref(pg), one, 1.0, one, None) == _lib.PN_ERR_ARG
        assert "g_weight" in lib.pn_last_error().decode()
        assert lib.pn_pagg_backward_paths(None, ctypes.byref(a), None, pw, ctypes.byref(pg), None) == _lib.PN_ERR_ARG
        assert "g_weight" in lib.pn_last_error().decode()


def test_as_path_weights_refuses_by_default_and_accepts_with_the_opt_in():
    from pathnet_amd import modules
    w = torch.ones(12, dtype=torch.float64, requires_grad=True)
    with pytest.raises(ValueError, match="requires grad.*path_grad"):
        modules.as_path_weights(w, 3, 4)
    got = modules.as_path_weights(w, 3, 4, path_grad=True)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 4) and got.requires_grad
    got.sum().backward()
    assert w.grad.dtype == torch.float64 and tuple(w.grad.shape) == (12,) and bool((w.grad == 1).all())


def test_every_entry_of_the_modules_takes_the_keyword():
    import pathnet_amd
    for cls in (pathnet_amd.PathNet, pathnet_amd.PathNet_homo, pathnet_amd.PAGG):
        for fn in (cls.forward, cls.encode, cls.forward_loss):
            par = inspect.signature(fn).parameters["path_grad"]
            assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is False, (cls, fn)
