"""tests/contrast_ref.py against torch and against itself, on the CPU: the restatement is the loss a user would write, its
bounds decide every named wrong implementation on the GPU case table, `hits` is decidable wherever it is compared exactly,
and the library's host-side contract (workspace size, tiles, refusals) holds without a GPU."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import contrast_ref as ref

GRID = [(tau, intra) for tau in ref.TAUS for intra in (0, 1)]


def torch_loss(A, B, tau, intra, live):
    """the torch composition of the same formula (F.normalize, cat, mm, masked logsumexp), fp64, live pairs given"""
    S = A.shape[0]
    z = torch.nn.functional.normalize(torch.cat((A, B)), dim=1, eps=0.0)
    live2 = torch.cat((live, live))
    s = z @ z.t() / tau
    r = torch.arange(2 * S)
    mask = live2[:, None] & live2[None, :] & (r[:, None] != r[None, :])
    if not intra:
        mask &= (r[:, None] >= S) != (r[None, :] >= S)
    lse = torch.logsumexp(s.masked_fill(~mask, float("-inf")), dim=1)
    pos = s[r, (r + S) % (2 * S)]
    rows = torch.where(live2, lse - pos, torch.zeros_like(pos))
    return rows.sum() / (2 * live.sum())


@pytest.mark.parametrize("kind", ("random", "dup", "valid"))
def test_reference_equals_torch_fp64_autograd(kind):
    for (S, D), (tau, intra) in itertools.product(((2, 3), (9, 5), (40, 17)), GRID):
        A, B, valid = ref.make_inputs(kind, S, D)
        want = ref.reference(A, B, tau, intra, valid, g=0.75)
        At, Bt = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (A, B))
        loss = torch_loss(At, Bt, tau, intra, torch.from_numpy(want.live[:S].copy()))
        (0.75 * loss).backward()
        assert abs(loss.item() - want.loss) <= 1e-12 * abs(want.loss)
        for got, w in ((At.grad.numpy(), want.dA), (Bt.grad.numpy(), want.dB)):
            assert np.abs(got - w).max() <= 1e-12 * np.abs(w).max(), (kind, S, D, tau, intra)


def test_reference_is_symmetric_under_swapping_the_views():
    for kind, (tau, intra) in itertools.product(("random", "mix"), GRID):
        A, B, valid = ref.make_inputs(kind, 23, 7)
        x, y = ref.reference(A, B, tau, intra, valid), ref.reference(B, A, tau, intra, valid)
        assert abs(x.loss - y.loss) <= 1e-13 * abs(x.loss) and (x.M, x.bad, x.hits) == (y.M, y.bad, y.hits)
        assert np.allclose(x.dA, y.dB, rtol=1e-12, atol=1e-15) and np.allclose(x.dB, y.dA, rtol=1e-12, atol=1e-15)
        assert np.allclose(x.row_loss[:23], y.row_loss[23:], rtol=1e-12, atol=1e-15)


def outside(right, wrong):
    """the wrong variant's loss or some gradient element lies outside the bound around the right one"""
    ta, tb = ref.tol_grad(right)
    return (abs(wrong.loss - right.loss) > ref.tol_loss(right) or bool((np.abs(wrong.dA - right.dA) > ta).any())
            or bool((np.abs(wrong.dB - right.dB) > tb).any()))


@pytest.mark.parametrize("variant", ref.VARIANTS)
def test_the_bound_decides_every_named_wrong_variant(variant):
    caught = total = 0
    for (kind, S, D, _), (tau, intra) in itertools.product(ref.case_table(), GRID):
        A, B, valid, right = ref.case(kind, S, D, tau, intra)
        if right.M == 0:
            continue
        hit = outside(right, ref.reference(A, B, tau, intra, valid, variant=variant))
        total += 1
        caught += hit
        if variant in ("nopartner", "intra") and S >= 2 and right.M >= 2:
            assert hit, (variant, kind, S, D, tau, intra)
    assert caught >= 1, variant
    print("%s: outside the bound on %d of %d cases" % (variant, caught, total))


def test_hits_is_decidable_wherever_it_is_compared_exactly():
    worst = np.inf
    for (kind, S, D, exact), (tau, intra) in itertools.product(ref.case_table(), GRID):
        if not exact:
            continue
        right = ref.case(kind, S, D, tau, intra)[3]
        ok, ratio = ref.hits_decidable(right)
        assert ok, "%s S=%d D=%d tau=%g intra=%d: a margin is %g x the bound" % (kind, S, D, tau, intra, ratio)
        worst = min(worst, ratio)
    print("the smallest margin is %.3g x the bound" % worst)


def test_case_table_covers_the_tile_edges():
    rt, ct, kc = ref.tiles()
    assert rt >= 2 and ct >= 2 and kc >= 2
    sizes = {S for _, S, _, _ in ref.case_table()}
    for t in (rt, ct):
        assert {t // 2 - 1, t // 2, t // 2 + 1} <= sizes            # 2S at t - 2, t, t + 2
        assert {t - 1, t, t + 1} <= sizes                           # S at t - 1, t, t + 1
    assert any(2 * ct < 2 * S < 3 * ct for S in sizes)              # three column tiles, the last one partial
    assert {1, 2, kc - 1, kc, kc + 1, 2 * kc + 1} <= {D for _, _, D, _ in ref.case_table()}
    assert set(ref.KINDS) <= {k for k, _, _, _ in ref.case_table()}
    assert max(2 * S for S in sizes) <= 3 * ct + 1


def lib():
    from pathnet_amd import _lib
    return _lib, _lib.load()


def test_workspace_bound_is_linear_in_S():
    _lib, L = lib()
    for S, D in itertools.product((0, 1, 1299, 10 ** 6), (1, 256, 8192)):
        n = ctypes.c_int64(-1)
        assert L.pn_contrast_workspace_bytes(S, D, ctypes.byref(n)) == _lib.PN_OK
        assert 0 <= n.value <= 2 * (2 * S * D * 4) + 64 * 2 * S + 4096 and n.value % 8 == 0, (S, D, n.value)


def test_every_argument_refusal_comes_before_any_device_call():
    """no context, no device: a call that got past its argument checks would fail differently (or crash)"""
    _lib, L = lib()
    n = ctypes.c_int64(-7)
    for S, D in ((-1, 4), (2 ** 30, 4), (5, 0), (5, 8193)):
        assert L.pn_contrast_workspace_bytes(S, D, ctypes.byref(n)) == _lib.PN_ERR_ARG and n.value == -7
    assert L.pn_contrast_workspace_bytes(5, 4, None) == _lib.PN_ERR_ARG
    assert L.pn_contrast_tiles(None) == _lib.PN_ERR_ARG
    buf = np.zeros(1 << 16, np.uint8)
    p = ctypes.c_void_p(buf.ctypes.data + (-buf.ctypes.data) % 8)
    odd = ctypes.c_void_p(p.value + 4)
    out = _lib.ContrastOut(p, p, p, p)
    big = 1 << 15

    def fwd(S=4, D=3, tau=0.5, A=p, B=p, lda=3, ldb=3, ws=p, nbytes=big, o=out):
        return L.pn_contrast_forward(None, A, lda, B, ldb, S, D, tau, 1, None, ws, nbytes, ctypes.byref(o) if o else None, None)

    def bwd(S=4, D=3, tau=0.5, A=p, B=p, lda=3, ldb=3, ws=p, nbytes=big, g=p, dA=p, dB=p):
        return L.pn_contrast_backward(None, A, lda, B, ldb, S, D, tau, 1, ws, nbytes, g, dA, dB, None)

    bad = [dict(S=-1), dict(S=2 ** 30), dict(D=0), dict(D=8193), dict(tau=0.0), dict(tau=-1.0), dict(tau=float("inf")),
           dict(tau=float("nan")), dict(A=None), dict(B=None), dict(ws=None), dict(ws=odd), dict(nbytes=64), dict(lda=2),
           dict(ldb=2)]
    for kw in bad:
        assert fwd(**kw) == _lib.PN_ERR_ARG, kw
        assert bwd(**kw) == _lib.PN_ERR_ARG, kw
    assert fwd(o=None) == _lib.PN_ERR_ARG
    for kw in (dict(g=None), dict(dA=None), dict(dB=None)):
        assert bwd(**kw) == _lib.PN_ERR_ARG, kw
    assert not buf.any()
