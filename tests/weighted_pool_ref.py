"""fp64 reference of the aggregators' pooling with per-path weights (pn_path_weights), for the tests.

Everything up to the paths' final hidden states is the oracle's (oracle/pagg_oracle.py, run in float64); only the pooling and
the classifier are redone here, as include/pathnet_hip.h defines them: with the live weights w_m of a pooling group
(a weight that is no finite positive number counts as 0), Om = sum w_m, kappa = W / Om ("sum") or 1 ("count"), 0 for Om = 0,

    pagg    pooled = (1/W) sum kappa w_m h_m
    homo    pooled = (1/W) sum kappa w_m (1 + s_m) h_m
    hetero  pooled = (1/W) sum kappa a_m h_m,   a_m = w_m e_m / sum_k w_k e_k,   e_m = exp(l_m - max_k l_k), l = LeakyReLU(score)

The weights are indexed by sequence slot q like ids without the last axis; the plan says which group and member a slot is.
Gradients come from autograd.  Also here: the NumPy statement of pn_path_multiplicity."""
import numpy as np
import torch

from oracle import pagg_oracle as po


def live(omega):
    """the weights as the kernels count them: 0 unless finite and positive"""
    om = torch.as_tensor(omega, dtype=torch.float64)
    return torch.where(torch.isfinite(om) & (om > 0), om, torch.zeros_like(om))


def forward(variant, params, X, ids, codes, sel, W, L, omega=None, norm="sum", cell=None, drop_seq=None, drop_cls=None):
    """-> (logits [S, C], embedding [S, 2H], applied coefficient [S, W] in (group, member) order), float64.
    omega: [S, W] / [S * W] by sequence slot, or None for all ones."""
    dt = torch.float64
    _, it = po.forward(variant, params, X, ids, codes, sel, W, L, drop_seq=drop_seq, dtype=dt, return_intermediates=True, cell=cell)
    h, y, Xh = it["h"], it["y"], it["Xh"]
    g = {k: v.to(dt) for k, v in params.items()}
    S = len(sel)
    H = h.shape[1]
    _, _, group, member, ego = po.plan(variant, np.asarray(ids), np.asarray(codes), S, W, L)
    order = torch.from_numpy(np.argsort(group * W + member, kind="stable"))
    hg = h[order].view(S, W, H)
    om = live(torch.ones(S * W) if omega is None else torch.as_tensor(omega).reshape(-1))[order].view(S, W)
    Om = om.sum(1, keepdim=True)
    kappa = (W / Om.clamp(min=1e-300)) if norm == "sum" else torch.ones_like(Om)
    kappa = torch.where(Om > 0, kappa, torch.zeros_like(Om))
    if variant == "pagg":
        coef = kappa * om
    else:
        ego_rows = (y[:, 0, :] if variant == "homo" else Xh[torch.from_numpy(ego)])[order].view(S, W, H)
        sc = po._lin(torch.cat([hg, ego_rows], dim=-1), g["attw.weight"], g["attw.bias"]).view(S, W)
        if variant == "homo":
            coef = kappa * om * (1.0 + sc)
        else:
            l = torch.nn.functional.leaky_relu(sc, 0.01)
            e = om * torch.exp(l - l.max(dim=1, keepdim=True).values)
            den = e.sum(1, keepdim=True)
            coef = kappa * torch.where(den > 0, e / den.clamp(min=1e-300), torch.zeros_like(e))
    pooled = (coef.unsqueeze(-1) * hg).sum(1) / W
    emb = torch.cat([Xh[torch.as_tensor(np.asarray(sel), dtype=torch.long)], pooled], dim=1)
    layer1 = emb if drop_cls is None else emb * drop_cls.to(dt)
    return po._lin(layer1, g["fc2.weight"], g["fc2.bias"]), emb, coef


def to_slots(variant, gm):
    """weights given per (pooling group, member) [S, W] -> the [S, W] array by sequence slot that the call takes"""
    gm = np.asarray(gm)
    S, W = gm.shape
    return gm.T.reshape(S, W).copy() if variant == "hetero" else gm.copy()      # hetero: slot q = member * S + group


def path_multiplicity_np(ids, codes=None):
    """mult[..., j] = paths of the row equal to path j (ids, and codes when given) if j is the first of them, else 0"""
    ids = np.asarray(ids)
    W, L = ids.shape[-2:]
    key = ids.reshape(-1, W, L).astype(np.int64)
    if codes is not None:
        key = np.concatenate([key, np.asarray(codes).reshape(-1, W, L).astype(np.int64)], axis=2)
    mult = np.zeros(key.shape[:2], np.float32)
    for r in range(key.shape[0]):
        eq = (key[r][:, None, :] == key[r][None, :, :]).all(-1)        # [W, W]
        first = ~np.tril(eq, -1).any(1)
        mult[r] = np.where(first, eq.sum(1), 0)
    return mult.reshape(ids.shape[:-1])
