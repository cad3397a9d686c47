"""pn_knn_search / pn_knn_vote on the GPU, through the C ABI, against the NumPy restatement tests/knn_ref.py.

As in test_gpu_contrast.py every input, workspace and output sits between two guard bands of 0xFF bytes that must come back
untouched, outputs start as 0xFF themselves, and with a row stride above D the padding behind every input row is NaN.

Held to (bounds and their derivation: knn_ref's docstring): every case of the table by the tolerant checker, which leaves no
row out; the integer cases of the dot metric and planted identical rows bit for bit; the outputs byte-equal for every work
split, for a row queried alone or in a batch, and between runs; the vote's labels, confusion matrix and skipped count exactly
where the margins decide them (test_knn_ref_host.py shows they do) and its probabilities inside their bound; every refusal
with the outputs untouched.
"""
import ctypes

import numpy as np
import pytest
import torch

import knn_ref as ref
import test_gpu_ensemble as tge
from test_gpu_contrast import padded

pytestmark = pytest.mark.gpu

Guarded, lib_ctx = tge.Guarded, tge.lib_ctx


def guarded_of(a):
    a = np.array(a, order="C")        # (a writable copy: the shared cases are read-only)
    g = Guarded(max(a.nbytes, 4))
    if a.nbytes:
        g.payload[:a.nbytes].copy_(torch.from_numpy(a.view(np.uint8).reshape(-1)))
    return g


def read(g, dtype, shape):
    """the first prod(shape) items of a Guarded payload (which holds at least 4 bytes, also for an empty array)"""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return g.payload[:n].cpu().numpy().view(dtype).reshape(shape).copy()


def gpu_knn(Q, X, k, metric, valid=None, exclude=None, splits=0, pad=3):
    """-> (ref.Result of numpy outputs, the raw bytes of everything written)"""
    _lib, lib, ctx, stream = lib_ctx()
    (Sq, D), N = Q.shape, X.shape[0]
    need = ctypes.c_int64(-1)
    _lib.check(lib.pn_knn_workspace_bytes(Sq, N, D, k, splits, ctypes.byref(need)))
    assert need.value % 8 == 0
    ld = D + pad
    qg, xg = padded(Q, ld), padded(X, ld)
    vg = guarded_of(np.asarray(valid, np.uint8)) if valid is not None else None
    eg = guarded_of(np.asarray(exclude, np.int64)) if exclude is not None else None
    ws = Guarded(need.value)
    bufs = dict(index=Guarded(max(8 * Sq * k, 4)), score=Guarded(max(4 * Sq * k, 4)), count=Guarded(max(4 * Sq, 4)),
                counts=Guarded(16))
    out = _lib.KnnOut(*(bufs[f].ptr() for f in _lib.KnnOut.FIELDS))
    _lib.check(lib.pn_knn_search(ctx, qg.ptr(), ld, Sq, xg.ptr(), ld, N, D, k, metric, vg.ptr() if vg else None,
                                 eg.ptr() if eg else None, splits, ws.ptr(), need.value, ctypes.byref(out), stream))
    torch.cuda.synchronize()
    for g in (qg, xg, ws) + tuple(bufs.values()) + tuple(x for x in (vg, eg) if x is not None):
        assert g.intact()
    got = ref.Result(index=read(bufs["index"], np.int64, (Sq, k)), score=read(bufs["score"], np.float32, (Sq, k)),
                     count=read(bufs["count"], np.int32, (Sq,)), counts=read(bufs["counts"], np.int64, (2,)))
    raw = torch.cat([bufs[f].payload[:n] for f, n in (("index", 8 * Sq * k), ("score", 4 * Sq * k), ("count", 4 * Sq),
                                                       ("counts", 16))]).clone()
    return got, raw


@pytest.mark.parametrize("i", range(len(ref.CASES)))
def test_case_table(i):
    """every case of the table is an acceptable answer for the tolerant checker; guard bands intact"""
    Q, X, valid, exclude, k, metric, t = ref.case(i)
    got, _ = gpu_knn(Q, X, k, metric, valid, exclude)
    assert ref.check(got, Q, X, k, metric, valid, exclude, t) is None, ref.CASES[i]
    if ref.CASES[i][0] == "self":           # no query is its own neighbour
        assert (got.index != np.asarray(exclude)[:, None]).all()


@pytest.mark.parametrize("i", range(len(ref.INT_CASES)))
def test_integer_dot_products_are_exact(i):
    Q, X, k, index, score, _ = ref.int_case(i)
    got, _ = gpu_knn(Q, X, k, ref.DOT)
    assert (got.index == index).all(), ref.INT_CASES[i]
    held = index >= 0
    assert (got.score[held].view(np.int32) == (score[held].astype(np.float32) + np.float32(0)).view(np.int32)).all()
    assert np.isneginf(got.score[~held]).all() and (got.count == held.sum(axis=1)).all()


@pytest.mark.parametrize("metric", (ref.COSINE, ref.DOT))
def test_identical_bank_rows_come_back_in_index_order(metric):
    """the same row at 0, 127, 128 and N - 1 (both sides of a column tile's edge and of the splits): equal score bits, ascending
    index, ahead of everything else"""
    N, D = 400, 17
    rng = np.random.default_rng(3)
    X = rng.standard_normal((N, D)).astype(np.float32)
    v = (3.0 * rng.standard_normal(D)).astype(np.float32)
    twins = [0, 127, 128, N - 1]
    X[twins] = v
    Q = np.stack([v, rng.standard_normal(D).astype(np.float32)])
    for splits in (0, 1, 3):
        got, _ = gpu_knn(Q, X, 8, metric, splits=splits)
        assert got.index[0, :4].tolist() == twins
        assert len(set(got.score[0, :4].view(np.int32).tolist())) == 1 and got.score[0, 4] < got.score[0, 3]
        assert ref.check(got, Q, X, 8, metric) is None


def test_negative_zero_scores_tie_with_positive_zero():
    """dot metric, D = 16 (one full K chunk: no + 0 padding joins the chain): every product of bank rows 1, 4, 7 ... is a tiny
    negative number that underflows, so the fma chain rounds to -0.0 and stays there; rows 0, 3, 6 ... give +0.0 by underflow
    from above and rows 2, 5, 8 ... are zero rows.  All tie: ascending index, and every score comes back as +0.0.  (Ranked by
    their bits, the -0.0 rows would come after all the others.)  One row with a real negative score comes last of all."""
    N, D = 130, 16
    X = np.zeros((N, D), np.float32)
    X[0::3], X[1::3] = np.float32(1e-30), np.float32(-1e-30)
    X[5] = -1.0
    Q = np.full((2, D), 1e-30, np.float32)
    assert np.signbit(np.float32(1e-30) * np.float32(-1e-30)) and np.float32(1e-30) * np.float32(-1e-30) == 0
    for splits in (0, 1):
        got, _ = gpu_knn(Q, X, 64, ref.DOT, splits=splits, pad=0)
        want = [i for i in range(N) if i != 5][:64]
        assert (got.index == np.array(want)[None, :]).all() and (got.count == 64).all()
        assert (got.score.view(np.int32) == 0).all()         # +0.0, whatever the sign of the chain's zero
    every, _ = gpu_knn(Q[:1], X, 64, ref.DOT, exclude=np.array([0]), valid=(np.arange(N) % 3 == 1) | (np.arange(N) == 5))
    assert every.index[0, :43].tolist() == list(range(1, N, 3)) and every.index[0, 43] == 5 and every.count[0] == 44
    assert (every.score[0, :43].view(np.int32) == 0).all() and every.score[0, 43] < 0


def test_the_work_split_changes_no_bit():
    for i in (4, 7, 13):        # N = 257 and 400, k = 64 and 32, dead rows, bank_valid, exclude
        Q, X, valid, exclude, k, metric, _ = ref.case(i)
        _, base = gpu_knn(Q, X, k, metric, valid, exclude, splits=0)
        for splits in (1, 2, 3, 7):
            _, raw = gpu_knn(Q, X, k, metric, valid, exclude, splits=splits)
            assert torch.equal(raw, base), (ref.CASES[i], splits)
        _, flat = gpu_knn(Q, X, k, metric, valid, exclude, splits=0, pad=0)
        assert torch.equal(flat, base)          # the stride changes no bit


def test_a_row_alone_equals_the_row_in_the_batch_and_two_runs_agree():
    Q, X, valid, exclude, k, metric, _ = ref.case(4)
    got, raw = gpu_knn(Q, X, k, metric, valid, exclude)
    other = torch.empty(3 * 1000 * 1000 + 17, dtype=torch.uint8, device="cuda").fill_(7)        # moves the allocations
    again, raw2 = gpu_knn(Q, X, k, metric, valid, exclude)
    assert torch.equal(raw, raw2)
    del other
    for r in (0, 63, 64, 129):
        one, _ = gpu_knn(Q[r:r + 1], X, k, metric, valid, exclude[r:r + 1])
        assert (one.index[0] == got.index[r]).all() and (one.score[0].view(np.int32) == got.score[r].view(np.int32)).all()
        assert one.count[0] == got.count[r]


def test_cosine_scores_are_symmetric_bit_for_bit():
    """knn(X, X): the score of (i -> j) has the bits of (j -> i) wherever both lists hold the pair"""
    X = ref.make_inputs("plain", 1, 257, 33)[1]
    got, _ = gpu_knn(X, X, 32, ref.COSINE, exclude=np.arange(257))
    seen = {}
    for i in range(257):
        for j, s in zip(got.index[i], got.score[i].view(np.int32)):
            seen[(i, int(j))] = int(s)
    pairs = [(a, b) for (a, b) in seen if (b, a) in seen]
    assert len(pairs) > 500 and all(seen[(a, b)] == seen[(b, a)] for a, b in pairs)


def test_empty_sides():
    rng = np.random.default_rng(0)
    Q, X = rng.standard_normal((5, 6)).astype(np.float32), rng.standard_normal((9, 6)).astype(np.float32)
    Q[1, 2] = np.nan
    X[3] = np.inf
    got, _ = gpu_knn(Q, X[:0], 4, ref.COSINE)
    assert (got.index == -1).all() and np.isneginf(got.score).all() and not got.count.any() and got.counts.tolist() == [1, 0]
    got, _ = gpu_knn(Q[:0], X, 4, ref.COSINE)
    assert got.counts.tolist() == [0, 1]
    got, _ = gpu_knn(Q[:0], X[:0], 4, ref.DOT)
    assert got.counts.tolist() == [0, 0]


# ---- the vote -------------------------------------------------------------------------------------------------------------------
def gpu_vote(index, score, count, bank_labels, C, T, labels=None):
    _lib, lib, ctx, stream = lib_ctx()
    Sq, k = index.shape
    ins = [guarded_of(np.asarray(a, dt)) for a, dt in ((index, np.int64), (score, np.float32), (count, np.int32),
                                                       (bank_labels, np.int64))]
    lg = guarded_of(np.asarray(labels, np.int64)) if labels is not None else None
    prob, label = Guarded(8 * Sq * C), Guarded(8 * Sq)
    conf, skipped = Guarded(8 * C * C, fill=0), Guarded(8, fill=0)
    _lib.check(lib.pn_knn_vote(ctx, ins[0].ptr(), ins[1].ptr(), ins[2].ptr(), Sq, k, ins[3].ptr(), len(bank_labels), C, T,
                               lg.ptr() if lg else None, prob.ptr(), label.ptr(), conf.ptr() if lg else None,
                               skipped.ptr() if lg else None, stream))
    torch.cuda.synchronize()
    for g in ins + [prob, label, conf, skipped] + ([lg] if lg else []):
        assert g.intact()
    return ref.Result(prob=prob.numpy(np.float64, (Sq, C)), label=label.numpy(np.int64, (Sq,)),
                      confusion=conf.numpy(np.int64, (C, C)), skipped=skipped.numpy(np.int64, (1,)))


@pytest.mark.parametrize("i", range(len(ref.VOTE_CASES)))
def test_vote_table(i):
    index, score, count, bank_labels, C, T, labels, want = ref.vote_case(i)
    got = gpu_vote(index, score, count, bank_labels, C, T, labels)
    err = np.abs(got.prob - want.prob)
    assert np.isfinite(got.prob).all() and (err <= want.tol).all(), (err / np.maximum(want.tol, 1e-300)).max()
    assert (got.prob[want.label < 0] == 0).all() and (got.label[want.label < 0] == -1).all()
    assert (want.margin > 1.0).all()        # (every row of the table is decided: test_knn_ref_host.py)
    assert (got.label == want.label).all()
    assert (got.confusion == want.confusion).all() and got.skipped[0] == want.skipped[0]
    again = gpu_vote(index, score, count, bank_labels, C, T, labels)
    assert (again.prob.view(np.int64) == got.prob.view(np.int64)).all() and (again.label == got.label).all()


def test_vote_after_a_search_and_without_labels():
    """the search's own outputs feed the vote: planted clusters are classified exactly; without labels nothing but prob and
    label is written"""
    rng = np.random.default_rng(9)
    C, per, D = 3, 50, 16
    centres = 4.0 * np.eye(C, D)
    X = (np.repeat(centres, per, axis=0) + 0.3 * rng.standard_normal((C * per, D))).astype(np.float32)
    y = np.repeat(np.arange(C), per)
    got, _ = gpu_knn(X, X, 10, ref.COSINE, exclude=np.arange(C * per))
    vote = gpu_vote(got.index, got.score, got.count, y, C, 0.07, labels=y)
    assert (vote.label == y).all() and (vote.confusion == per * np.eye(C, dtype=np.int64)).all() and vote.skipped[0] == 0
    bare = gpu_vote(got.index, got.score, got.count, y, C, 0.07)
    assert (bare.label == y).all() and not bare.confusion.any() and not bare.skipped.any()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    _lib, lib, ctx, stream = lib_ctx()
    Sq, N, D, k = 5, 9, 6, 4
    rng = np.random.default_rng(1)
    qg, xg = padded(rng.standard_normal((Sq, D)).astype(np.float32), D), padded(rng.standard_normal((N, D)).astype(np.float32), D)
    ws = Guarded(1 << 16)
    bufs = dict(index=Guarded(8 * Sq * k), score=Guarded(4 * Sq * k), count=Guarded(4 * Sq), counts=Guarded(16))
    out = _lib.KnnOut(*(bufs[f].ptr() for f in _lib.KnnOut.FIELDS))
    good = dict(Q=qg.ptr(), ldq=D, Sq=Sq, X=xg.ptr(), ldx=D, N=N, D=D, k=k, metric=0, splits=0, ws=ws.ptr(), ws_bytes=1 << 16,
                out=ctypes.byref(out))
    bad = [dict(Sq=-1), dict(Sq=2 ** 31), dict(N=-1), dict(N=2 ** 31), dict(D=0), dict(D=8193), dict(k=0), dict(k=ref.MAX_K + 1),
           dict(metric=2), dict(metric=-1), dict(splits=-1), dict(splits=1025), dict(ldq=D - 1), dict(ldx=D - 1), dict(Q=None),
           dict(X=None), dict(ws=None), dict(ws_bytes=ref.workspace_bytes(Sq, N, D, k) - 1),
           dict(ws=ctypes.c_void_p(ws.ptr().value + 4)), dict(out=None)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.pn_knn_search(ctx, a["Q"], a["ldq"], a["Sq"], a["X"], a["ldx"], a["N"], a["D"], a["k"], a["metric"], None, None,
                               a["splits"], a["ws"], a["ws_bytes"], a["out"], stream)
        assert rc == _lib.PN_ERR_ARG, change
    torch.cuda.synchronize()
    assert all(g.untouched() for g in bufs.values()) and ws.untouched()
    # the vote
    index, score, count, bank_labels, C, T, labels, _ = ref.vote_case(0)
    Sq, k = index.shape
    ins = [guarded_of(a) for a in (index, score, count, bank_labels, labels)]
    outs = [Guarded(8 * Sq * C), Guarded(8 * Sq), Guarded(8 * C * C), Guarded(8)]
    good = dict(index=ins[0].ptr(), score=ins[1].ptr(), count=ins[2].ptr(), Sq=Sq, k=k, bank=ins[3].ptr(), N=len(bank_labels), C=C,
                T=T, labels=ins[4].ptr())
    bad = [dict(Sq=-1), dict(N=2 ** 31), dict(k=0), dict(k=ref.MAX_K + 1), dict(C=0), dict(C=4097), dict(T=0.0), dict(T=-1.0),
           dict(T=float("nan")), dict(index=None), dict(score=None), dict(count=None), dict(bank=None), dict(labels=None)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.pn_knn_vote(ctx, a["index"], a["score"], a["count"], a["Sq"], a["k"], a["bank"], a["N"], a["C"], a["T"],
                             a["labels"], outs[0].ptr(), outs[1].ptr(), outs[2].ptr(), outs[3].ptr(), stream)
        assert rc == _lib.PN_ERR_ARG, change
    torch.cuda.synchronize()
    assert all(g.untouched() for g in outs)
