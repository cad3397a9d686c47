"""The fp16 BPTT's step boundaries (pathnet_amd/csrc/pn_seqh.hip, seq_bwdh_kernel) at the shapes where they can go wrong.

The kernel requests a tile's index entries, dhn and the saved values of the last step together and unconditionally -- a
padded row of a ragged tile reads the tile's last live row and is zeroed afterwards -- and scatters dx through one of
three straight-line bodies (explicit mask / keep bits / no dropout) whose row ids and slots are 16-byte reads of
step-major tables.  What that must survive:

  paths per launch  P = S W in {1, 31, 32, 33, 65}: a single row (every clamped load reads row 0), a ragged only tile, a
                    whole tile, whole tiles followed by a tile of one row;
  path length       L in {1, 2, 4}: at 1 the prologue's loads are the only ones and the merging step the only step;
  hidden size       32 (one wave; L = 4 takes the rolled remainder of the index staging), 96 (not a power of two: step 0
                    scatters like every other step), 128;
  cells             LSTM, GRU, tanh RNN;  dropout off, built in at 0.7, explicit masks;  the homo plan (step 0 merges runs
                    of equal rows) and the hetero plan (it does not);
  merging           a tile whose 32 paths start at one node (one run) and one whose 32 start rows all differ (32 runs).

References: without dropout and with explicit masks the CPU oracle (oracle/pagg_oracle.py) in fp32 under the suite's
contract (logits within 1e-5, gradients by tests/gradcheck.py).  The built-in masks are drawn inside the kernels from a
seed the oracle cannot see: there the reference is the bf16 x 3 kernels of pn_seq3.hip on the same module, inputs and
seed (they draw the same masks and are themselves held to the oracle by tests/test_gpu_seqh.py), under that file's
bounds for the pair (logits 2e-6, gradients rel 1e-5)."""
import numpy as np
import pytest
import torch
from gradcheck import ZERO_OK_HETERO, assert_grads_close

from oracle import pagg_oracle as po

pytestmark = pytest.mark.gpu

N, F, C = 300, 40, 4


def _module(variant, cell, H, L, drop):
    import pathnet_amd
    if variant == "pagg":
        m = pathnet_amd.PAGG(F, H, C, N, dropout=drop, cell=cell)
    else:
        cls = {"homo": pathnet_amd.PathNet_homo, "hetero": pathnet_amd.PathNet}[variant]
        m = cls(F, H, C, L, dropout=drop, cell=cell)
    m = m.cuda().train()
    m.seq_math = "f16x2"
    return m


def _inputs(S, W, L, H, seed, keep=0.5):
    g = torch.Generator().manual_seed(seed + 4)
    rng = np.random.default_rng(seed + 1)
    X = torch.rand(N, F, generator=g)
    sel = np.sort(rng.choice(N, S, replace=False))
    ids = rng.integers(0, N, (S, W, L)).astype(np.int32)
    ids[:, :, 0] = sel[:, None]
    codes = rng.integers(0, L, (S, W, L)).astype(np.uint8)
    mask_seq = (torch.rand(L, S * W, H, generator=g) < keep).float() / keep
    mask_cls = (torch.rand(S, 2 * H, generator=g) < keep).float() / keep
    Gout = torch.randn(S, C, generator=g)
    return X, sel, ids, codes, mask_seq, mask_cls, Gout


def _hip(m, X, sel, ids, codes, Gout, W, L, masks=None, seed=7):
    S = len(sel)
    m._mask_seq, m._mask_cls = (masks[0].cuda(), masks[1].cuda()) if masks else (None, None)
    node_mask = np.zeros(N, bool)
    node_mask[sel] = True
    torch.manual_seed(seed)         # the module draws its dropout seed from torch's generator
    m.zero_grad(set_to_none=True)
    out = m(X.cuda(), torch.as_tensor(ids.reshape(S, W * L).astype(np.int64)), W, L, node_mask,
            torch.as_tensor(codes.astype(np.int64)), None)
    out.backward(Gout.cuda())
    torch.cuda.synchronize()
    return out.detach().cpu(), {k: v.grad.detach().cpu() for k, v in m.named_parameters()}


def _oracle(variant, cell, m, X, sel, ids, codes, Gout, W, L, masks):
    params = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    want = po.forward(variant, params, X, ids, codes, sel, W, L, drop_seq=masks[0] if masks else None,
                      drop_cls=masks[1] if masks else None, cell=cell)
    want.backward(Gout)
    # (autograd leaves .grad None for a parameter the case never touches -- a distance layer no path uses: exactly zero)
    return want.detach(), {k: params[k].grad if params[k].grad is not None else torch.zeros_like(params[k])
                           for k, _ in m.named_parameters()}


def _zero_ok(variant):
    return ZERO_OK_HETERO if variant == "hetero" else ()


# (variant, cell, H, S, W, L, explicit masks?)
ORACLE_CASES = [
    ("homo", None, 128, 1, 1, 4, True),         # P = 1: rows_here = 1, every clamped load reads row 0
    ("homo", None, 128, 31, 1, 4, False),       # P = 31: one ragged tile, 31 runs of one row
    ("homo", None, 128, 1, 32, 4, True),        # P = 32: a tile whose 32 paths start at ONE node (one run of 32)
    ("homo", None, 128, 32, 1, 4, False),       # P = 32: a tile whose 32 start rows all differ
    ("homo", None, 128, 11, 3, 4, True),        # P = 33: a whole tile and a tile of one row; a run crosses the tile edge
    ("homo", None, 128, 13, 5, 2, False),       # P = 65, L = 2
    ("homo", None, 128, 13, 5, 1, True),        # L = 1: the merging step is the only step
    ("hetero", None, 128, 11, 3, 4, True),      # the hetero plan: step 0 scatters like every other step
    ("hetero", None, 128, 13, 5, 1, False),
    ("homo", "gru", 128, 11, 3, 4, True),
    ("homo", "rnn", 128, 13, 5, 2, False),
    ("pagg", None, 96, 11, 3, 4, True),         # tanh RNN at H = 96: no step-0 merge, odd unit count
    ("homo", None, 96, 13, 5, 4, True),
    ("homo", "gru", 96, 31, 1, 2, False),
    ("homo", None, 32, 13, 5, 4, True),         # one wave; 32 L = 128 index entries for 64 threads
    ("homo", "gru", 32, 11, 3, 4, False),
    ("pagg", None, 32, 1, 1, 4, True),          # (PAGG has its four distance layers: L = 4 only)
    ("homo", "rnn", 32, 1, 1, 1, True),         # the smallest launch there is
    ("hetero", None, 32, 13, 5, 4, True),
    ("homo", None, 32, 1, 32, 2, False),
]


@pytest.mark.parametrize("variant,cell,H,S,W,L,explicit", ORACLE_CASES)
def test_bptt_edges_match_the_oracle(variant, cell, H, S, W, L, explicit):
    m = _module(variant, cell, H, L, 0.5 if explicit else 0.0)
    X, sel, ids, codes, ms, mc, G = _inputs(S, W, L, H, seed=11)
    masks = (ms, mc) if explicit else None
    out, g = _hip(m, X, sel, ids, codes, G, W, L, masks)
    want, wg = _oracle(variant, cell, m, X, sel, ids, codes, G, W, L, masks)
    assert not torch.isnan(out).any()
    assert (out - want).abs().max().item() < 1e-5
    assert_grads_close(g, wg, zero_ok=_zero_ok(variant))


# built-in dropout at 0.7: (variant, cell, H, S, W, L)
BUILTIN_CASES = [
    ("homo", None, 128, 13, 5, 4),
    ("homo", None, 128, 1, 1, 1),               # one path, one step
    ("homo", None, 128, 1, 32, 4),              # one run of 32
    ("homo", None, 128, 32, 1, 4),              # 32 runs of one
    ("homo", None, 128, 31, 1, 2),
    ("hetero", None, 128, 11, 3, 2),
    ("homo", "gru", 96, 13, 5, 4),
    ("homo", "rnn", 96, 11, 3, 1),
    ("pagg", None, 32, 31, 1, 4),
    ("homo", None, 32, 8, 4, 4),
    ("hetero", "gru", 32, 13, 5, 2),
]


@pytest.mark.parametrize("variant,cell,H,S,W,L", BUILTIN_CASES)
def test_bptt_edges_with_built_in_dropout_match_the_bf16_kernels(variant, cell, H, S, W, L):
    m = _module(variant, cell, H, L, 0.7)
    X, sel, ids, codes, _, _, G = _inputs(S, W, L, H, seed=12)
    m.seq_math = "bf16x3"
    ref_out, ref_g = _hip(m, X, sel, ids, codes, G, W, L)
    m.seq_math = "f16x2"
    out, g = _hip(m, X, sel, ids, codes, G, W, L)
    assert not torch.isnan(out).any()
    assert (out - ref_out).abs().max().item() <= 2e-6
    assert_grads_close(g, ref_g, rel=1e-5, zero_ok=_zero_ok(variant))


@pytest.mark.parametrize("variant,cell,H,S,W,L,drop", [
    ("homo", None, 128, 13, 5, 4, 0.7),         # keep bits, a ragged last tile of one row
    ("homo", None, 128, 1, 32, 4, 0.0),         # no dropout
    ("hetero", None, 32, 11, 3, 4, 0.7),
    ("homo", "rnn", 96, 31, 1, 1, 0.7),
])
def test_deterministic_mode_is_bit_reproducible_and_agrees_with_the_default(variant, cell, H, S, W, L, drop):
    """the fixed-order backward stores dx rows instead of adding them: two runs are bit-equal, and equal to the default
    (atomic) mode within the gradient bound"""
    m = _module(variant, cell, H, L, drop)
    X, sel, ids, codes, _, _, G = _inputs(S, W, L, H, seed=13)
    m.deterministic = False
    out0, g0 = _hip(m, X, sel, ids, codes, G, W, L)
    m.deterministic = True
    out1, g1 = _hip(m, X, sel, ids, codes, G, W, L)
    out2, g2 = _hip(m, X, sel, ids, codes, G, W, L)
    assert torch.equal(out1, out2) and torch.equal(out0, out1)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    assert_grads_close(g1, g0, zero_ok=_zero_ok(variant))


def test_explicit_masks_in_deterministic_mode_match_the_oracle():
    """the explicit-mask body crossed with the storing scatter"""
    variant, cell, H, S, W, L = "homo", None, 128, 11, 3, 4
    m = _module(variant, cell, H, L, 0.5)
    m.deterministic = True
    X, sel, ids, codes, ms, mc, G = _inputs(S, W, L, H, seed=14)
    out, g = _hip(m, X, sel, ids, codes, G, W, L, (ms, mc))
    want, wg = _oracle(variant, cell, m, X, sel, ids, codes, G, W, L, (ms, mc))
    assert (out - want).abs().max().item() < 1e-5
    assert_grads_close(g, wg)
