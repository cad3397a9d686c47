"""pn_contrast_forward / pn_contrast_backward on the GPU, through the C ABI, against the NumPy restatement tests/contrast_ref.py.

As in test_gpu_ensemble.py every input, workspace, output and gradient sits between two guard bands of 0xFF bytes that must
come back untouched, and outputs start as 0xFF themselves; with lda > D the padding behind every input row is NaN.

Held to (bounds and their derivation: contrast_ref's docstring): row_loss, loss, dA and dB element by element inside the derived
bounds; counts exactly; hits exactly wherever the case table says the margins decide it (test_contrast_ref_host.py proves
they do); dead rows' gradients exactly zero; two runs bit-equal.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import contrast_ref as ref
import test_gpu_ensemble as tge

pytestmark = pytest.mark.gpu

Guarded, lib_ctx = tge.Guarded, tge.lib_ctx


def padded(X, ld):
    """[S, D] fp32 -> Guarded [S, ld] with NaN behind every row"""
    S, D = X.shape
    buf = np.full((S, ld), np.nan, np.float32)
    buf[:, :D] = X
    g = Guarded(max(buf.nbytes, 4))
    if buf.nbytes:
        g.payload[:buf.nbytes].copy_(torch.from_numpy(buf.view(np.uint8).reshape(-1)))
    return g


def gpu_contrast(A, B, tau, intra, valid=None, g=1.0, pad=0, backward=True):
    """-> (dict of numpy outputs, the raw bytes of everything written)"""
    _lib, lib, ctx, stream = lib_ctx()
    S, D = A.shape
    need = ctypes.c_int64(-1)
    _lib.check(lib.pn_contrast_workspace_bytes(S, D, ctypes.byref(need)))
    assert need.value <= 2 * (2 * S * D * 4) + 64 * 2 * S + 4096 and need.value % 8 == 0
    ld = D + pad
    ag, bg = padded(A, ld), padded(B, ld)
    vg = None
    if valid is not None:
        vg = Guarded(max(S, 1))
        vg.payload[:S].copy_(torch.from_numpy(np.array(valid, np.uint8)))
    ws = Guarded(need.value)
    bufs = dict(loss=Guarded(8), row_loss=Guarded(max(8 * S, 4)), hits=Guarded(8), counts=Guarded(16))
    out = _lib.ContrastOut(*(bufs[k].ptr() for k in _lib.ContrastOut.FIELDS))
    _lib.check(lib.pn_contrast_forward(ctx, ag.ptr(), ld, bg.ptr(), ld, S, D, tau, intra, vg.ptr() if vg is not None else None,
                                       ws.ptr(), need.value, ctypes.byref(out), stream))
    got = {}
    written = [bufs[k] for k in _lib.ContrastOut.FIELDS]
    if backward:
        gg = Guarded(4)
        gg.payload.copy_(torch.from_numpy(np.array([g], np.float32).view(np.uint8)))
        da, db = Guarded(max(4 * S * D, 4)), Guarded(max(4 * S * D, 4))
        _lib.check(lib.pn_contrast_backward(ctx, ag.ptr(), ld, bg.ptr(), ld, S, D, tau, intra, ws.ptr(), need.value, gg.ptr(),
                                            da.ptr(), db.ptr(), stream))
        torch.cuda.synchronize()
        assert gg.intact() and da.intact() and db.intact()
        if S:
            got.update(dA=da.numpy(np.float32, (S, D)), dB=db.numpy(np.float32, (S, D)))
        written += [da, db]
    torch.cuda.synchronize()
    for x in (ag, bg, ws) + tuple(bufs.values()) + ((vg,) if vg is not None else ()):
        assert x.intact()
    got.update(loss=float(bufs["loss"].numpy(np.float64, (1,))[0]), hits=int(bufs["hits"].numpy(np.int64, (1,))[0]),
               counts=bufs["counts"].numpy(np.int64, (2,)))
    if S:
        got["row_loss"] = bufs["row_loss"].numpy(np.float32, (2 * S,))
    raw = torch.cat([w.payload for w in written]).clone()
    return got, raw


def check(got, want, tag, hits_exact=True, g=1.0):
    """want: ref.reference(...) at the same g"""
    assert got["counts"].tolist() == [want.M, want.bad], (tag, got["counts"])
    if want.S == 0:
        assert got["loss"] == 0.0 and got["hits"] == 0
        return
    err = np.abs(got["row_loss"].astype(np.float64) - want.row_loss)
    tol = ref.tol_row_loss(want)
    assert np.isfinite(got["row_loss"]).all() and (err <= tol).all(), "%s: row_loss off by %g of its bound" % (
        tag, (err / tol).max())
    assert (got["row_loss"][~want.live] == 0).all(), tag
    assert abs(got["loss"] - want.loss) <= ref.tol_loss(want), "%s: loss off by %g of its bound" % (
        tag, abs(got["loss"] - want.loss) / ref.tol_loss(want))
    if hits_exact:
        assert got["hits"] == want.hits, (tag, got["hits"], want.hits)
    if "dA" in got:
        ta, tb = ref.tol_grad(want, g)
        for name, x, w, t in (("dA", got["dA"], want.dA, ta), ("dB", got["dB"], want.dB, tb)):
            assert np.isfinite(x).all(), (tag, name)
            e = np.abs(x.astype(np.float64) - w)
            assert (e <= t).all(), "%s: %s off by %g of its bound" % (tag, name, (e / np.maximum(t, 1e-300)).max())
            dead = ~want.live[:want.S]
            assert (x[dead] == 0).all(), (tag, name)


@pytest.mark.parametrize("tau", ref.TAUS)
@pytest.mark.parametrize("intra", (0, 1))
def test_case_table(tau, intra):
    """every (kind, S, D) of the table: row_loss, loss, dA, dB inside the bounds, counts and hits exact, guard bands intact"""
    for kind, S, D, hits_exact in ref.case_table():
        A, B, valid, want = ref.case(kind, S, D, tau, intra)
        got, _ = gpu_contrast(A, B, tau, intra, valid)
        check(got, want, (kind, S, D, tau, intra), hits_exact)


def test_a_single_pair():
    rng = np.random.default_rng(5)
    A, B = rng.standard_normal((1, 9)).astype(np.float32), rng.standard_normal((1, 9)).astype(np.float32)
    for tau in ref.TAUS:
        # intra = 0: the partner is the row's only term: loss and gradients within the bound of 0
        got, _ = gpu_contrast(A, B, tau, 0)
        want = ref.reference(A, B, tau, 0)
        assert want.loss == 0.0 and not want.dA.any() and not want.dB.any() and want.hits == 2
        check(got, want, ("S=1", tau, 0))
        # intra = 1: the same set (the row itself is never a term)
        got, _ = gpu_contrast(A, B, tau, 1)
        check(got, ref.reference(A, B, tau, 1), ("S=1", tau, 1))
    got, _ = gpu_contrast(np.zeros((0, 5), np.float32), np.zeros((0, 5), np.float32), 0.5, 1)
    assert got["loss"] == 0.0 and got["hits"] == 0 and not got["counts"].any()


@pytest.mark.parametrize("how", ("invalid", "nan"))
def test_no_live_pair(how):
    S, D = 37, 11
    A, B, _ = ref.make_inputs("random", S, D)
    valid = None
    if how == "invalid":
        valid = np.zeros(S, np.uint8)
    else:
        A = A.copy()
        A[:, 3] = np.nan
    for intra in (0, 1):
        got, _ = gpu_contrast(A, B, 0.5, intra, valid)
        assert got["loss"] == 0.0 and got["hits"] == 0
        assert got["counts"].tolist() == [0, 0 if how == "invalid" else S]
        assert not got["row_loss"].any() and not got["dA"].any() and not got["dB"].any()


@pytest.mark.parametrize("intra", (0, 1))
def test_dead_rows_take_no_part(intra):
    """a mix of invalid, NaN, inf and zero-norm rows: their gradients are exactly 0, and everything else equals the reference
    computed WITHOUT those rows"""
    rt, ct, kc = ref.tiles()
    S, D, tau = ct + 3, kc + 1, 0.5
    A, B, valid = ref.make_inputs("mix", S, D, seed=3)
    got, _ = gpu_contrast(A, B, tau, intra, valid)
    As, Bs, keep = ref.without_dead_rows(A, B, valid)
    assert 0 < len(keep) < S
    small = ref.reference(As, Bs, tau, intra)
    full = ref.reference(A, B, tau, intra, valid)
    assert got["counts"].tolist() == [len(keep), full.bad] and full.bad > 0
    dead = np.ones(S, bool)
    dead[keep] = False
    assert (got["dA"][dead] == 0).all() and (got["dB"][dead] == 0).all()
    assert (got["row_loss"][np.concatenate((dead, dead))] == 0).all()
    sub = dict(counts=np.array([small.M, small.bad]), loss=got["loss"], hits=got["hits"],
               row_loss=got["row_loss"][np.concatenate((keep, keep + S))], dA=got["dA"][keep], dB=got["dB"][keep])
    # (the bound's tile count is the full call's: evaluate it there)
    small.n = full.n
    check(sub, small, ("without the dead rows", intra))


def test_strided_inputs_and_zero_upstream_gradient():
    S, D, tau = 70, 19, 0.5
    A, B, valid = ref.make_inputs("valid", S, D)
    want = ref.reference(A, B, tau, 1, valid, g=-2.5)
    got, raw = gpu_contrast(A, B, tau, 1, valid, g=-2.5, pad=3)
    check(got, want, "lda = D + 3", g=-2.5)
    flat, raw2 = gpu_contrast(A, B, tau, 1, valid, g=-2.5)
    assert torch.equal(raw, raw2)           # the stride changes no bit
    zero, _ = gpu_contrast(A, B, tau, 1, valid, g=0.0, pad=3)
    assert not zero["dA"].any() and not zero["dB"].any()


def test_two_runs_give_the_same_bits():
    rt, ct, kc = ref.tiles()
    for (S, D), intra in itertools.product(((ct + 1, 2 * kc + 1), (rt + 1, kc)), (0, 1)):
        A, B, valid = ref.make_inputs("mix", S, D, seed=1)
        _, raw = gpu_contrast(A, B, 0.07, intra, valid)
        other = torch.empty(3 * 1000 * 1000 + 17 * S, dtype=torch.uint8, device="cuda").fill_(7)     # moves the allocations
        _, raw2 = gpu_contrast(A, B, 0.07, intra, valid)
        assert torch.equal(raw, raw2), (S, D, intra)
        del other


def test_scaling_a_view_by_a_power_of_two():
    """A * 4: the unit rows, and with them the loss, keep their bits; dA is the gradient of A divided by 4, bit for bit"""
    S, D = 45, 13
    A, B, _ = ref.make_inputs("random", S, D)
    for intra in (0, 1):
        one, _ = gpu_contrast(A, B, 0.5, intra)
        four, _ = gpu_contrast(A * np.float32(4), B, 0.5, intra)
        assert np.float64(one["loss"]).view(np.int64) == np.float64(four["loss"]).view(np.int64)
        assert (one["row_loss"].view(np.int32) == four["row_loss"].view(np.int32)).all()
        assert (four["dA"].view(np.int32) == (one["dA"] / np.float32(4)).view(np.int32)).all()
        assert (four["dB"].view(np.int32) == one["dB"].view(np.int32)).all()
