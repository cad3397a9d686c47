"""pn_ensemble_add / pn_ensemble_finish on the GPU, through the C ABI, against the NumPy restatement tests/ensemble_ref.py.

Every state and output buffer sits between two guard bands of 0xFF bytes (NaN as fp32 / fp64, -1 as an integer) that must
come back untouched; outputs start as 0xFF themselves, so an entry a call was to leave alone is seen to be left alone.

Held to (bounds and their derivation: ensemble_ref's docstring): votes, count, bad, label, vote_label, confusion, skipped
and status exactly; psum and hsum within the derived fp64 bound of the long-double evaluation; prob, confidence and
agreement within ONE fp32 ulp of the reference rounded to fp32; entropy and mutual_info within one ulp plus the fp64 bound of
their expression, which for these two is absolute and not negligible against the ulp of a small value.
"""
import ctypes

import numpy as np
import pytest
import torch

import ensemble_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 256
F32_OUT = ("prob", "confidence", "entropy", "mutual_info", "agreement")
I64_OUT = ("label", "vote_label", "confusion", "skipped")


class Guarded:
    """`nbytes` of device memory between two guard bands; fill: the payload's initial byte"""

    def __init__(self, nbytes, fill=0xFF):
        self.nbytes = int(nbytes)
        self.whole = torch.full((2 * GUARD + self.nbytes + (-self.nbytes) % 8,), 0xFF, dtype=torch.uint8, device="cuda")
        self.payload = self.whole[GUARD:GUARD + self.nbytes]
        if fill != 0xFF:
            self.payload.fill_(fill)

    def ptr(self):
        return ctypes.c_void_p(self.whole.data_ptr() + GUARD)

    def intact(self):
        w = self.whole
        return bool((w[:GUARD] == 0xFF).all()) and bool((w[GUARD + self.nbytes:] == 0xFF).all())

    def untouched(self):
        return self.intact() and bool((self.payload == 0xFF).all())

    def numpy(self, dtype, shape):
        return self.payload.cpu().numpy().view(dtype).reshape(shape).copy()


def lib_ctx():
    from pathnet_amd import _lib
    return _lib, _lib.load(), _lib.context("cuda"), _lib.stream_ptr("cuda")


def state_bytes(rows, C):
    _lib, lib, _, _ = lib_ctx()
    n = ctypes.c_int64(-1)
    _lib.check(lib.pn_ensemble_state_bytes(rows, C, ctypes.byref(n)))
    return n.value


def read_state(g, rows, C):
    raw = g.payload.cpu().numpy()
    o = 0
    psum = raw[o:o + 8 * rows * C].view(np.float64).reshape(rows, C).copy(); o += 8 * rows * C      # noqa: E702
    hsum = raw[o:o + 8 * rows].view(np.float64).copy(); o += 8 * rows                              # noqa: E702
    votes = raw[o:o + 4 * rows * C].view(np.int32).reshape(rows, C).copy(); o += 4 * rows * C      # noqa: E702
    count = raw[o:o + 4 * rows].view(np.int32).copy(); o += 4 * rows                               # noqa: E702
    bad = raw[o:o + 4 * rows].view(np.int32).copy(); o += 4 * rows                                 # noqa: E702
    assert o == len(raw)
    return ref.State(psum, hsum, votes, count, bad)


def gpu_add(state, x, rows, index=None, status=None):
    """x: numpy fp32 [R, S, C] -> one pn_ensemble_add into the Guarded state"""
    _lib, lib, ctx, stream = lib_ctx()
    R, S, C = x.shape
    xg = Guarded(x.nbytes)
    xg.payload.copy_(torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)))
    ig = None
    if index is not None:
        ig = Guarded(4 * S)
        ig.payload.copy_(torch.from_numpy(np.ascontiguousarray(index, np.int32).view(np.uint8).reshape(-1)))
    _lib.check(lib.pn_ensemble_add(ctx, xg.ptr(), R, S, C, ig.ptr() if ig is not None else None, rows, state.ptr(),
                                   status.ptr() if status is not None else None, stream))
    torch.cuda.synchronize()
    assert xg.intact() and (ig is None or ig.intact())


def gpu_finish(state, rows, C, subset=None, target=None, want=F32_OUT + I64_OUT):
    """-> ({name: numpy}, {name: Guarded})"""
    _lib, lib, ctx, stream = lib_ctx()
    n = rows if subset is None else len(subset)
    shapes = dict(prob=(n, C), label=(n,), vote_label=(n,), confidence=(n,), entropy=(n,), mutual_info=(n,), agreement=(n,),
                  confusion=(C, C), skipped=(2,))
    bufs, keep = {}, []
    for k in want:
        if k in ("confusion", "skipped"):
            if target is None:
                continue
            bufs[k] = Guarded(8 * int(np.prod(shapes[k])), fill=0)      # added to: the caller zeroes them
        else:
            bufs[k] = Guarded((4 if k in F32_OUT else 8) * int(np.prod(shapes[k])))
    out = _lib.EnsembleOut(*(bufs[k].ptr() if k in bufs else None for k in _lib.EnsembleOut.FIELDS))
    sg = tg = None
    if subset is not None:
        sg = Guarded(4 * n)
        sg.payload.copy_(torch.from_numpy(np.ascontiguousarray(subset, np.int32).view(np.uint8).reshape(-1)))
    if target is not None:
        tg = Guarded(8 * rows)
        tg.payload.copy_(torch.from_numpy(np.ascontiguousarray(target, np.int64).view(np.uint8).reshape(-1)))
    keep += [sg, tg]
    _lib.check(lib.pn_ensemble_finish(ctx, rows, C, state.ptr(), sg.ptr() if sg is not None else None,
                                      n if subset is not None else 0, tg.ptr() if tg is not None else None,
                                      ctypes.byref(out), stream))
    torch.cuda.synchronize()
    got = {k: g.numpy(np.float32 if k in F32_OUT else np.int64, shapes[k]) for k, g in bufs.items()}
    for k, g in bufs.items():
        assert g.intact(), k
    assert state.intact()
    return got, bufs


def check_state(got, x, rows, index):
    """exact members against the fp64 restatement, psum / hsum within the bound of the long-double one -> fp64 restatement"""
    R, S, C = x.shape
    lo, hi = ref.new_state(rows, C), ref.new_state(rows, C, np.longdouble)
    ref.add(lo, x, index)
    ref.add(hi, x, index)
    for f in ("votes", "count", "bad"):
        assert (getattr(got, f) == getattr(lo, f)).all(), f
    K = max(int(lo.count.max()), 1) if rows else 1
    e_p = np.abs(got.psum - hi.psum).astype(np.float64)
    tol = ref.tol_psum(hi.psum.astype(np.float64), C, K)
    assert (e_p <= tol).all(), "psum off by %g of its bound" % (e_p / tol).max()
    e_h = np.abs(got.hsum - hi.hsum).astype(np.float64)
    tol = ref.tol_hsum(hi.hsum.astype(np.float64), lo.count, C, K)
    assert (e_h <= tol).all(), "hsum off by %g of its bound" % (e_h / tol).max()
    return lo


def decidable(st, C, K):
    """rows whose label does not hang on a rounding: top-two margin of psum far above its bound, or an exact tie (bit-identical
    columns see identical operations on both sides)"""
    if C == 1:
        return np.ones(len(st.count), bool)
    top = np.sort(st.psum, axis=1)[:, -2:]
    margin = top[:, 1] - top[:, 0]
    return (margin == 0) | (margin > 8 * ref.tol_psum(top[:, 1], C, K)) | (st.count == 0)


def check_finish(got, st, C, subset=None, target=None):
    want = ref.finish(st, subset, target)
    row = np.arange(len(st.count)) if subset is None else np.asarray(subset, np.int64)
    inside = (row >= 0) & (row < len(st.count))
    K = max(int(st.count.max()), 1) if len(st.count) else 1
    ok = np.ones(len(row), bool)
    ok[inside] = decidable(st, C, K)[row[inside]]
    assert ok.all(), "the case holds %d rows whose label hangs on a rounding: choose another seed" % (~ok).sum()
    for k in ("label", "vote_label"):
        assert (got[k] == getattr(want, k)).all(), k
    for k in ("prob", "confidence", "agreement"):
        w = getattr(want, k)
        err = np.abs(got[k].astype(np.float64) - w.astype(np.float64))
        assert (err <= ref.ulp32(w)).all(), "%s: %g ulp" % (k, (err / ref.ulp32(w)).max())
    ent, hbar = want.exact
    rel_q = ref.rel_p(C) + (K + 1) * ref.U
    t_ent = ref.tol_entropy(ent, C, rel_q)
    n = np.maximum(np.where(inside, st.count[np.where(inside, row, 0)] if len(st.count) else 0, 0), 1)
    t_mi = t_ent + ref.tol_hsum(hbar * n, n, C, K) / n
    for k, extra in (("entropy", t_ent), ("mutual_info", t_mi)):
        w = getattr(want, k)
        err = np.abs(got[k].astype(np.float64) - w.astype(np.float64))
        assert (err <= ref.ulp32(w) + extra).all(), k
    if target is not None:
        assert (got["confusion"] == want.confusion).all() and (got["skipped"] == want.skipped).all()
    return want


@pytest.mark.parametrize("with_index", (False, True), ids=("identity", "index"))
@pytest.mark.parametrize("kind", ref.KINDS)
def test_case_table(kind, with_index):
    """every (C, S, R) of the table: one [R, S, C] call against the restatement, R single-sample calls bit-equal to it, a
    second run bit-equal to the first, and finish with targets that include -1 and C"""
    for C, S, R in ref.case_table():
        rng = np.random.default_rng(1000 * C + 10 * S + R)
        x = ref.make_logits(kind, R, S, C, seed=C * 7 + S * 3 + R)
        rows = S + 9 if with_index else S
        index = rng.permutation(rows)[:S].astype(np.int32) if with_index else None
        nb = state_bytes(rows, C)
        one, many, again = (Guarded(nb, fill=0) for _ in range(3))
        gpu_add(one, x, rows, index)
        for r in range(R):
            gpu_add(many, x[r:r + 1], rows, index)
        gpu_add(again, x, rows, index)
        assert one.intact() and many.intact() and again.intact(), (C, S, R)
        assert torch.equal(one.payload, many.payload), "(%d, %d, %d): R calls differ from one" % (C, S, R)
        assert torch.equal(one.payload, again.payload), "(%d, %d, %d): two runs differ" % (C, S, R)
        if S == 0 and rows == 0:
            assert nb == 0
            got, bufs = gpu_finish(one, rows, C)          # rows == 0: succeeds, writes nothing
            assert all(g.untouched() for g in bufs.values())
            continue
        st = check_state(read_state(one, rows, C), x, rows, index)
        target = rng.integers(-1, C + 1, size=rows).astype(np.int64)
        got, _ = gpu_finish(one, rows, C, target=target)
        check_finish(got, st, C, target=target)


def test_accumulate_across_calls_and_orders():
    """K samples in three calls (2 + 1 + 2) equal one pass over all five, bit for bit (the order is the same); the samples in
    another order agree within the bound"""
    for C, S in ((7, 130), (65, 33), (1025, 5)):
        x = ref.make_logits("normal", 5, S, C, seed=11)
        nb = state_bytes(S, C)
        one, parts, other = (Guarded(nb, fill=0) for _ in range(3))
        gpu_add(one, x, S)
        for a, b in ((0, 2), (2, 3), (3, 5)):
            gpu_add(parts, x[a:b], S)
        gpu_add(other, x[::-1], S)
        assert torch.equal(one.payload, parts.payload)
        a, b = read_state(one, S, C), read_state(other, S, C)
        assert (a.votes == b.votes).all() and (a.count == b.count).all()
        assert (np.abs(a.psum - b.psum) <= 2 * ref.tol_psum(a.psum, C, 5)).all()
        assert (np.abs(a.hsum - b.hsum) <= 2 * ref.tol_hsum(a.hsum, a.count, C, 5)).all()


def test_index_outside_the_state_is_skipped_and_counted():
    C, S, R, rows = 7, 70, 3, 40
    x = ref.make_logits("normal", R, S, C, seed=5)
    index = np.full(S, -1, np.int32)
    index[:rows] = np.random.default_rng(0).permutation(rows)
    index[rows:rows + 10] = rows + np.arange(10)            # just past the end
    index[-1] = 2 ** 31 - 1
    state, status = Guarded(state_bytes(rows, C), fill=0), Guarded(4, fill=0)
    gpu_add(state, x, rows, index, status)
    assert status.intact() and state.intact()
    want = ref.new_state(rows, C)
    assert status.numpy(np.int32, (1,))[0] == ref.add(want, x, index) == R * (S - rows)
    got = read_state(state, rows, C)
    assert (got.count == want.count).all() and (got.votes == want.votes).all() and (got.count == R).all()


def test_subset_target_and_optional_outputs():
    C, S, R = 5, 90, 4
    x = ref.make_logits("nonfinite", R, S, C, seed=8)
    state = Guarded(state_bytes(S, C), fill=0)
    gpu_add(state, x, S)
    st = check_state(read_state(state, S, C), x, S, None)
    rng = np.random.default_rng(2)
    target = rng.integers(0, C, size=S).astype(np.int64)
    target[::7], target[3::7] = -1, C
    subset = np.concatenate([rng.permutation(S)[:40], [5, 5, -1, S, 1]]).astype(np.int32)      # repeats and outsiders
    got, _ = gpu_finish(state, S, C, subset=subset, target=target)
    want = check_finish(got, st, C, subset=subset, target=target)
    assert want.skipped[0] > 0 and want.skipped[1] > 2 and got["label"][-3] == -1 and got["label"][-2] == -1
    # two subsets that split the rows: their confusion matrices add up to the whole state's
    a, _ = gpu_finish(state, S, C, subset=np.arange(0, S, 2, dtype=np.int32), target=target)
    b, _ = gpu_finish(state, S, C, subset=np.arange(1, S, 2, dtype=np.int32), target=target)
    whole, _ = gpu_finish(state, S, C, target=target)
    assert (a["confusion"] + b["confusion"] == whole["confusion"]).all()
    assert (a["skipped"] + b["skipped"] == whole["skipped"]).all()
    # an output that is not asked for is not written, and the others do not change
    few, bufs = gpu_finish(state, S, C, target=target, want=("label", "entropy", "confusion"))
    assert set(few) == {"label", "entropy", "confusion"}
    assert (few["label"] == whole["label"]).all() and (few["entropy"] == whole["entropy"]).all()
    assert (few["confusion"] == whole["confusion"]).all()


def test_empty_calls_write_nothing():
    _lib, lib, ctx, stream = lib_ctx()
    C = 7
    state = Guarded(state_bytes(12, C), fill=0)
    x = Guarded(64)
    assert lib.pn_ensemble_add(ctx, x.ptr(), 3, 0, C, None, 12, state.ptr(), None, stream) == 0            # S == 0
    assert lib.pn_ensemble_add(ctx, x.ptr(), 1, 0, C, None, 0, None, None, stream) == 0                    # rows == 0
    out_bufs = {k: Guarded(64) for k in ("prob", "label")}
    out = _lib.EnsembleOut(prob=out_bufs["prob"].ptr(), label=out_bufs["label"].ptr())
    assert lib.pn_ensemble_finish(ctx, 0, C, None, None, 0, None, ctypes.byref(out), stream) == 0          # rows == 0
    sub = Guarded(8)
    assert lib.pn_ensemble_finish(ctx, 12, C, state.ptr(), sub.ptr(), 0, None, ctypes.byref(out), stream) == 0   # empty subset
    torch.cuda.synchronize()
    assert state.intact() and bool((state.payload == 0).all())
    assert all(g.untouched() for g in out_bufs.values()) and x.untouched() and sub.untouched()


def test_python_ensemble_matches_the_abi():
    """pathnet_amd.Ensemble: add / result / reset / check= over the same kernels"""
    import pathnet_amd
    C, S, R, rows = 9, 50, 3, 64
    x = ref.make_logits("margin", R, S, C, seed=21)
    index = np.random.default_rng(3).permutation(rows)[:S].astype(np.int32)
    labels = np.random.default_rng(4).integers(0, C, size=rows)
    ens = pathnet_amd.Ensemble(rows, C, "cuda")
    xt = torch.from_numpy(x).cuda()
    ens.add(xt[0], index=torch.from_numpy(index), check=True).add(xt[1:], index=index)
    st = ref.new_state(rows, C)
    ref.add(st, x, index)
    assert (ens.count.cpu().numpy() == st.count).all() and (ens.votes.cpu().numpy() == st.votes).all()
    assert (np.abs(ens.psum.cpu().numpy() - st.psum) <= 2 * ref.tol_psum(st.psum, C, R)).all()
    pred = ens.result(labels=labels)
    want = ref.finish(st, target=labels)
    assert (pred.label.cpu().numpy() == want.label).all() and (pred.confusion.cpu().numpy() == want.confusion).all()
    assert (pred.count.cpu().numpy() == st.count).all() and pred.skipped.tolist() == want.skipped.tolist()
    part = ens.result(rows=torch.from_numpy(index[:7].astype(np.int64)))
    assert (part.label.cpu().numpy() == want.label[index[:7]]).all() and part.confusion is None
    assert (part.count.cpu().numpy() == R).all()
    s = pred.summary()
    conf = want.confusion
    assert s["accuracy"] == pytest.approx(np.trace(conf) / conf.sum()) and s["rows"] == rows and s["valid_rows"] == S
    assert s["unlabelled_rows"] == rows - S and s["bad_share"] == 0.0
    with pytest.raises(ValueError):
        ens.add(xt[0], index=np.zeros(S, np.int32), check=True)        # a row named twice
    with pytest.raises(ValueError):
        ens.add(xt[0, :, :5])
    ens.reset()
    assert int(ens.count.sum()) == 0 and float(ens.psum.abs().sum()) == 0.0
    with pytest.raises(pathnet_amd._lib.PnError):
        pathnet_amd.Ensemble(4, 5000, "cuda")


def test_add_inside_a_captured_graph():
    """nothing is read back and nothing allocated inside add: a captured add replays, and two replays are two adds"""
    import pathnet_amd
    C, S, rows = 7, 33, 40
    x = torch.from_numpy(ref.make_logits("normal", 2, S, C, seed=9)).cuda()
    index = torch.from_numpy(np.random.default_rng(1).permutation(rows)[:S].astype(np.int32)).cuda()
    eager = pathnet_amd.Ensemble(rows, C, "cuda").add(x, index=index).add(x, index=index)
    ens = pathnet_amd.Ensemble(rows, C, "cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ens.add(x, index=index)             # warm-up on a side stream, as torch asks before a capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ens.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ens.add(x, index=index)
    torch.cuda.synchronize()
    assert int(ens.count.sum()) == 0        # captured, not run
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(ens.state, eager.state) and (ens.count[index.long()] == 4).all()
