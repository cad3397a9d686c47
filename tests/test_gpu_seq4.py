"""The two-stage weight-gradient GEMM of the bf16 x 3 arithmetic at hidden size 128 (pn_seq4.hip, context knob PN_SEQ4 bit 2,
on by default in that mode) against the generic one (wgrad3_kernel, pn_seq3.hip) on the same module, inputs and dropout seed,
and against the CPU oracle.  It replaces autograd's weight gradient of nn.LSTM (/root/reference/PathNet_run.py:164,195,265,351):
logits within 1e-5, gradients within 3e-5 of each tensor's largest element (tests/gradcheck.py).  (The 128-path forward and
BPTT that shared the file were experiments that measured slower; removed in round 6, profiles/HISTORY_r1_r4.md.)
The kernel's K-tile, split-count, ragged-tail and micro-batch edges are held to the fp64 oracle by tests/test_gpu_wgrad_edges.py."""
import os

import numpy as np
import pytest
import torch
from gradcheck import ZERO_OK_HETERO, assert_grads_close

from oracle import pagg_oracle as po

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore_env():
    from pathnet_amd import _lib
    old = {k: os.environ.get(k) for k in ("PN_SEQ_MATH",)}
    knobs = {k: _lib.get_knob(k) for k in ("PN_SEQ4",)}
    os.environ["PN_SEQ_MATH"] = "bf16x3"        # these kernels are bf16 x 3 variants: the fp16 default never dispatches them
    yield
    for k, v in knobs.items():
        _lib.set_knob(k, v)
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _case(variant, S, W, L, cell=None, drop=0.5, N=400, F=48, C=5, seed=0):
    import pathnet_amd
    g = torch.Generator().manual_seed(seed)
    cls = {"homo": pathnet_amd.PathNet_homo, "hetero": pathnet_amd.PathNet}[variant]
    torch.manual_seed(seed)
    m = cls(F, 128, C, L, dropout=drop, cell=cell).cuda().train()
    X = torch.rand(N, F, generator=g).cuda()
    sel = torch.randperm(N, generator=g)[:S].sort().values.to(torch.int32)
    ids = torch.randint(0, N, (S, W, L), generator=g).to(torch.int32)
    ids[:, :, 0] = sel[:, None]
    codes = torch.randint(0, L, (S, W, L), generator=g).to(torch.uint8)
    G = torch.randn(S, C, generator=g).cuda()
    return m, X, ids.cuda(), codes.cuda(), sel.cuda(), G


def _run(case, mask, seed=7):
    m, X, ids, codes, sel, G = case
    from pathnet_amd import _lib
    _lib.set_knob("PN_SEQ4", mask)
    torch.manual_seed(seed)          # the module draws its dropout seed from torch's generator
    m.zero_grad(set_to_none=True)
    out = m(X, ids, ids.shape[1], ids.shape[2], sel, codes, None)
    out.backward(G)
    torch.cuda.synchronize()
    return out.detach().clone(), {k: v.grad.detach().clone() for k, v in m.named_parameters()}


@pytest.mark.parametrize("variant,S,W,L,cell,drop", [
    ("homo", 97, 7, 4, None, 0.5),          # 679 paths: full tiles and a ragged one, for both tile widths
    ("homo", 1, 1, 4, None, 0.5),           # a single path
    ("homo", 64, 8, 4, None, 0.0),          # whole tiles, no dropout
    ("homo", 40, 9, 6, None, 0.5),          # path length 6 (configs[4])
    ("homo", 40, 9, 1, None, 0.5),          # one step: no recurrent products at all
    ("homo", 97, 7, 4, "gru", 0.5),         # GRU on the four gate slots
    ("hetero", 97, 7, 4, None, 0.5),        # the hetero index plan
])
def test_two_stage_weight_gradient_matches_the_generic_one(variant, S, W, L, cell, drop):
    case = _case(variant, S, W, L, cell, drop)
    ref_out, ref_g = _run(case, 0)
    out, g = _run(case, 4)
    assert not torch.isnan(out).any()
    assert (out - ref_out).abs().max().item() <= 1e-5
    assert_grads_close(g, ref_g, zero_ok=ZERO_OK_HETERO if variant == "hetero" else ())


def test_two_stage_weight_gradient_matches_the_oracle():
    """forward and every gradient against the CPU oracle with the same explicit dropout masks"""
    import pathnet_amd
    torch.manual_seed(1)
    N, F, H, C, S, W, L = 300, 40, 128, 4, 70, 11, 4
    g = torch.Generator().manual_seed(5)
    m = pathnet_amd.PathNet_homo(F, H, C, L, dropout=0.5).cuda().train()
    X = torch.rand(N, F, generator=g)
    sel = np.sort(np.random.default_rng(2).choice(N, S, replace=False))
    ids = np.random.default_rng(3).integers(0, N, (S, W, L)).astype(np.int32)
    ids[:, :, 0] = sel[:, None]
    codes = np.random.default_rng(4).integers(0, L, (S, W, L)).astype(np.uint8)
    keep = 0.5
    mask_seq = (torch.rand(L, S * W, H, generator=g) < keep).float() / keep
    mask_cls = (torch.rand(S, 2 * H, generator=g) < keep).float() / keep
    m._mask_seq, m._mask_cls = mask_seq.cuda(), mask_cls.cuda()
    from pathnet_amd import _lib
    _lib.set_knob("PN_SEQ4", 4)
    mask = np.zeros(N, bool)
    mask[sel] = True
    out = m(X.cuda(), torch.as_tensor(ids.reshape(S, W * L).astype(np.int64)), W, L, mask,
            torch.as_tensor(codes.astype(np.int64)), None)
    Gout = torch.randn(S, C, generator=g)
    out.backward(Gout.cuda())
    params = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    want = po.forward("homo", params, X, ids, codes, sel, W, L, drop_seq=mask_seq, drop_cls=mask_cls)
    assert (out.detach().cpu() - want.detach()).abs().max().item() < 1e-5
    want.backward(Gout)
    assert_grads_close({k: v.grad for k, v in m.named_parameters()}, {k: params[k].grad for k, _ in m.named_parameters()})
