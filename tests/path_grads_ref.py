"""fp64 reference of the gradients at the aggregators' per-path interface (pn_path_grads), for the tests.

Logits, embedding and the applied coefficient are tests/weighted_pool_ref.forward's, which is differentiable in `omega` as it
stands: a weight that is no finite positive number goes through torch.where, so it gets the gradient 0, and so does every
weight of a group without a live path.  Added here: the paths' final hidden states [S, W, H] in the order encode() returns
them -- member j of row s is sequence slot s * W + j (homo / PAGG) or j * S + s (hetero: the reference's scrambled batch, as
tests/test_gpu_encode.oracle builds it) -- from a second run of the oracle over the same leaves.  Gradients are autograd's."""
import numpy as np
import torch

from oracle import pagg_oracle as po
import weighted_pool_ref as wref


def leaves(state, X, omega=None):
    """({parameter name: fp32 leaf}, X leaf, omega as an fp64 leaf or None) -- all on the CPU, all requiring grad"""
    pr = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in state.items()}
    Xo = X.detach().cpu().clone().requires_grad_(True)
    om = None if omega is None else torch.as_tensor(np.asarray(omega), dtype=torch.float64).clone().requires_grad_(True)
    return pr, Xo, om


def forward(variant, params, X, ids, codes, sel, W, L, omega=None, norm="sum", cell=None, path_state=True):
    """-> (logits [S, C], embedding [S, 2H], applied coefficient [S, W], path states [S, W, H] or None), float64"""
    out, emb, coef = wref.forward(variant, params, X, ids, codes, sel, W, L, omega, norm, cell=cell)
    if not path_state:
        return out, emb, coef, None
    _, it = po.forward(variant, params, X, ids, codes, sel, W, L, dtype=torch.float64, return_intermediates=True, cell=cell)
    S = len(sel)
    s, j = np.meshgrid(np.arange(S), np.arange(W), indexing="ij")
    q = j * S + s if variant == "hetero" else s * W + j
    ps = it["h"][torch.as_tensor(q.reshape(-1))].view(S, W, -1)
    return out, emb, coef, ps


def grads(names, pr, Xo, om, loss):
    """{name: gradient} of `loss` for the parameters `names`, "X" and -- with om -- "path_weights" (zeros where autograd
    reached nothing)"""
    ts = [pr[k] for k in names] + [Xo] + ([om] if om is not None else [])
    # (a loss that depends on no leaf at all -- unweighted PAGG's constant coefficients -- has no graph: all zeros)
    gs = torch.autograd.grad(loss, ts, retain_graph=True, allow_unused=True) if loss.requires_grad else [None] * len(ts)
    gs = [torch.zeros_like(t) if g is None else g for t, g in zip(ts, gs)]
    ref = dict(zip(list(names) + ["X"] + (["path_weights"] if om is not None else []), gs))
    return ref
