"""pn_explain_groups / pn_explain_totals on the GPU, through the C ABI, against the NumPy restatement tests/explain_ref.py.

Every buffer sits between two guard bands of 0xFF bytes that must come back untouched, and outputs start as 0xFF themselves
(test_gpu_ensemble.Guarded).  Held to (bounds and their derivation: explain_ref's docstring): present, flip, target_used and
status exactly -- the inputs are drawn so that no two logits an argmax compares are closer than 1e-3 in the reference itself
-- and every fp32 output within ONE fp32 ulp of the long-double reference rounded to fp32 plus the derived fp64 bound of its
expression.
"""
import ctypes

import numpy as np
import pytest
import torch

import explain_ref as ref
from test_gpu_ensemble import Guarded, lib_ctx

pytestmark = pytest.mark.gpu

F32_OUT = ("full", "contribution", "drop_logits", "keep_logits", "drop_delta", "keep_gain")
ALL_OUT = F32_OUT + ("flip", "present", "target_used")
DTYPES = dict(flip=np.uint8, present=np.int32, target_used=np.int64)


def upload(a):
    a = np.ascontiguousarray(a)
    g = Guarded(a.nbytes)
    if a.nbytes:
        g.payload.copy_(torch.from_numpy(a.view(np.uint8).reshape(-1)))
    return g


def padded(a, ld):
    """rows of `a` (last axis) at a leading dimension of ld, the padding NaN: it must not be read"""
    out = np.full(a.shape[:-1] + (ld,), np.nan, a.dtype)
    out[..., :a.shape[-1]] = a
    return out


def gpu_groups(case, want=ALL_OUT, ld_state=None, ld_ego=None, ld_w=None, rows=None, with_status=True):
    """-> ({name: numpy}, status [2] or None).  rows: a slice of the case's rows"""
    _lib, lib, ctx, stream = lib_ctx()
    sl = slice(None) if rows is None else rows
    state, coef, ego, group = case.state[sl], case.coef[sl], case.ego[sl], case.group[sl]
    weight = None if case.weight is None else case.weight[sl]
    target = None if case.target is None else case.target[sl]
    S, W, H = state.shape
    C, G = case.fc2_w.shape[0], case.G
    ld_state, ld_ego, ld_w = ld_state or H, ld_ego or H, ld_w or 2 * H
    ins = dict(state=upload(padded(state, ld_state)), coef=upload(coef), ego=upload(padded(ego, ld_ego)),
               fc2_w=upload(padded(case.fc2_w, ld_w)), fc2_b=upload(case.fc2_b), group=upload(group.astype(np.int32)))
    if weight is not None:
        ins["weight"] = upload(weight)
    if target is not None:
        ins["target"] = upload(target.astype(np.int64))
    shapes = dict(full=(S, C), contribution=(S, W, C), drop_logits=(S, G, C), keep_logits=(S, G, C), drop_delta=(S, G),
                  keep_gain=(S, G), flip=(S, G), present=(S, G), target_used=(S,))
    bufs = {k: Guarded(int(np.prod(shapes[k])) * np.dtype(DTYPES.get(k, np.float32)).itemsize) for k in want}
    out = _lib.ExplainOut(*(bufs[k].ptr() if k in bufs else None for k in _lib.ExplainOut.FIELDS))
    status = Guarded(8, fill=0) if with_status else None
    p = lambda k: ins[k].ptr() if k in ins else None         # noqa: E731
    _lib.check(lib.pn_explain_groups(ctx, S, W, H, C, G, p("state"), ld_state, p("coef"), p("ego"), ld_ego, p("fc2_w"), ld_w,
                                     p("fc2_b"), p("weight"), p("group"), case.norm, case.renorm, p("target"),
                                     ctypes.byref(out), status.ptr() if status else None, stream))
    torch.cuda.synchronize()
    for k, g in list(ins.items()) + list(bufs.items()):
        assert g.intact(), k
    got = {k: g.numpy(DTYPES.get(k, np.float32), shapes[k]) for k, g in bufs.items()}
    if S == 0:
        assert all(g.untouched() for g in bufs.values())
    st = None
    if status is not None:
        assert status.intact()
        st = status.numpy(np.int32, (2,))
    return got, st


def check(got, st, case, rows=None, report=None):
    """every output against the long-double restatement; -> the fp64 restatement"""
    lo, hi = ref.run(case), ref.run(case, np.longdouble)
    sl = slice(None) if rows is None else rows
    if lo.full[sl].size and case.fc2_w.shape[0] > 1:
        assert ref.min_gap(lo) >= 1e-3, "the case holds logits closer than 1e-3: choose another seed"
    for k in ("flip", "present", "target_used"):
        if k in got:
            assert (got[k] == getattr(lo, k)[sl]).all(), k
    if st is not None and rows is None:
        assert st.tolist() == lo.status.tolist()
    for k in F32_OUT:
        if k not in got:
            continue
        want = ref.f32(getattr(hi, k)[sl])
        tol = ref.ulp32(want) + hi.tol[k][sl]
        nan = np.isnan(want)
        assert (np.isnan(got[k]) == nan).all(), k
        err = np.abs(got[k].astype(np.float64) - want.astype(np.float64))
        err[nan] = 0
        assert (err <= np.where(nan, 1, tol)).all(), "%s off by %g of its tolerance" % (k, (err / tol)[~nan].max())
        if report is not None and err.size:
            report[k] = max(report.get(k, 0.0), float((err / np.where(nan, 1, tol)).max()))
    return lo


@pytest.mark.parametrize("idx", range(len(ref.shape_table())))
def test_shape_table(idx):
    """one sweep per axis around W = 5, H = 32, C = 3, and both sides of every boundary of the work split: the route the library
    reports is the documented one, every output is inside its bound, and a second run leaves the same bits"""
    _lib, lib, _, _ = lib_ctx()
    sh = ref.shape_table()[idx]
    route = (ctypes.c_int32 * 4)()
    _lib.check(lib.pn_explain_route(sh["S"], sh["W"], sh["H"], sh["C"], sh["G"], route))
    assert list(route) == ref.route(**sh)
    case = ref.make_case(seed=100 + idx, renorm=idx % 2, norm=(idx // 2) % 2, **sh)
    got, st = gpu_groups(case)
    if sh["S"] == 0:
        return
    check(got, st, case)
    again, _ = gpu_groups(case)
    for k in ALL_OUT:
        assert got[k].tobytes() == again[k].tobytes(), k


@pytest.mark.parametrize("norm", (ref.NORM_SUM, ref.NORM_COUNT))
@pytest.mark.parametrize("renorm", (0, 1))
def test_norms_weights_and_targets(norm, renorm):
    """both norms, renorm on and off; weights NULL against all ones (the same bits); dead members; group ids outside [0, G);
    a target of the caller's against the argmax; targets out of range"""
    sh = dict(S=9, W=7, H=33, C=5, G=4)
    case = ref.make_case(seed=11, norm=norm, renorm=renorm, weights=False, **sh)
    got, st = gpu_groups(case)
    check(got, st, case)
    ones, _ = gpu_groups(case._replace(weight=np.ones((9, 7), np.float32)))
    for k in ALL_OUT:
        assert got[k].tobytes() == ones[k].tobytes(), k
    dead = ref.make_case(seed=12, norm=norm, renorm=renorm, weights=True, **sh)
    assert (~np.isfinite(dead.weight)).any() and (dead.weight == 0).any() and (dead.group == -1).any() and (dead.group == 4).any()
    check(*gpu_groups(dead), dead)
    free = dead._replace(target=None)
    got, st = gpu_groups(free)
    lo = check(got, st, free)
    assert (got["target_used"] == lo.full.argmax(1)).all()
    tgt = dead.target.copy()
    tgt[[1, 4]] = (5, -3)
    off = dead._replace(target=tgt)
    got, st = gpu_groups(off)
    check(got, st, off)
    assert st.tolist() == [2, 0] and (got["drop_delta"][[1, 4]] == 0).all() and (got["flip"][[1, 4]] == 0).all()
    gpu_groups(off, with_status=False)                       # a NULL status is not written to


def test_leading_dimensions():
    """ld_state / ld_ego / ld_w beyond H / 2H (odd ones: no 16-byte loads) give the bits of the packed call; the padding is NaN"""
    case = ref.make_case(S=4, W=6, H=32, C=3, G=3, seed=21)
    packed, _ = gpu_groups(case)
    check(packed, None, case)
    for lds in ((36, 40, 72), (33, 35, 67), (32, 32, 65)):
        got, _ = gpu_groups(case, ld_state=lds[0], ld_ego=lds[1], ld_w=lds[2])
        for k in ALL_OUT:
            assert got[k].tobytes() == packed[k].tobytes(), (k, lds)


def test_each_output_is_optional():
    case = ref.make_case(S=5, W=5, H=32, C=3, G=3, seed=22)
    whole, _ = gpu_groups(case)
    for leave in ALL_OUT:
        got, _ = gpu_groups(case, want=tuple(k for k in ALL_OUT if k != leave))
        for k in got:
            assert got[k].tobytes() == whole[k].tobytes(), (leave, k)
    got, st = gpu_groups(case, want=("drop_delta", "flip"))            # the scores need no logits stored
    assert got["drop_delta"].tobytes() == whole["drop_delta"].tobytes() and (got["flip"] == whole["flip"]).all()
    gpu_groups(case, want=())


@pytest.mark.parametrize("where", ("state", "coef", "ego"))
def test_a_non_finite_entry_makes_exactly_that_row_bad(where):
    case = ref.make_case(S=6, W=5, H=32, C=3, G=3, seed=23)
    clean, _ = gpu_groups(case)
    a = getattr(case, where).copy()
    a[(2, 4, 31) if where == "state" else (2, 4)] = {"state": np.inf, "coef": np.nan, "ego": -np.inf}[where]
    hurt = case._replace(**{where: a})
    got, st = gpu_groups(hurt)
    check(got, st, hurt)
    assert st.tolist() == [0, 1]
    keep = np.arange(6) != 2
    for k in ALL_OUT:
        assert got[k][keep].tobytes() == clean[k][keep].tobytes(), k
    for k in F32_OUT:
        assert np.isnan(got[k][2]).all(), k
    assert (got["flip"][2] == 0).all() and (got["present"][2] == clean["present"][2]).all()


def test_rows_split_over_two_calls_leave_the_same_bits():
    case = ref.make_case(S=11, W=40, H=128, C=7, G=40, seed=24, renorm=1)
    whole, _ = gpu_groups(case)
    check(whole, None, case)
    a, _ = gpu_groups(case, rows=slice(0, 4))
    b, _ = gpu_groups(case, rows=slice(4, 11))
    for k in ALL_OUT:
        assert np.concatenate([a[k], b[k]]).tobytes() == whole[k].tobytes(), k


def test_argument_refusals():
    _lib, lib, ctx, stream = lib_ctx()
    buf = Guarded(4096)
    out = _lib.ExplainOut()
    route = (ctypes.c_int32 * 4)()

    def call(S=1, W=2, H=4, C=3, G=2, ld_state=4, ld_ego=4, ld_w=8, norm=0, renorm=0, state=buf.ptr(), group=buf.ptr(),
             out=ctypes.byref(out)):
        return lib.pn_explain_groups(ctx, S, W, H, C, G, state, ld_state, buf.ptr(), buf.ptr(), ld_ego, buf.ptr(), ld_w, buf.ptr(),
                                     None, group, norm, renorm, None, out, None, stream)
    for kw in (dict(S=-1), dict(S=2 ** 31), dict(W=0), dict(W=1025), dict(G=0), dict(G=1025), dict(H=0), dict(H=4097), dict(C=0),
               dict(C=1025), dict(ld_state=3), dict(ld_ego=3), dict(ld_w=7), dict(norm=2), dict(renorm=2), dict(state=None),
               dict(group=None), dict(out=None)):
        assert call(**kw) == _lib.PN_ERR_ARG, kw
    assert call(S=0, state=None, group=None) == 0                     # S == 0: nothing is read, nothing launched
    assert lib.pn_explain_route(1, 0, 4, 3, 2, route) == _lib.PN_ERR_ARG
    assert lib.pn_explain_route(1, 2, 4, 3, 2, None) == _lib.PN_ERR_ARG
    t = lambda **kw: lib.pn_explain_totals(ctx, kw.get("S", 1), kw.get("G", 2), kw.get("dd", buf.ptr()), buf.ptr(), buf.ptr(),   # noqa: E731
                                           buf.ptr(), kw.get("rows"), kw.get("n", 0), kw.get("tot", buf.ptr()), stream)
    for kw in (dict(S=-1), dict(G=0), dict(G=1025), dict(n=3), dict(n=-1, rows=buf.ptr()), dict(dd=None), dict(tot=None)):
        assert t(**kw) == _lib.PN_ERR_ARG, kw
    assert t(S=0, dd=None, tot=None) == 0 and t(rows=buf.ptr(), n=0, tot=None) == 0
    torch.cuda.synchronize()
    assert buf.untouched()


def gpu_totals(tot, dd, kg, flip, present, rows=None):
    _lib, lib, ctx, stream = lib_ctx()
    S, G = dd.shape
    ins = [upload(a) for a in (dd.astype(np.float32), kg.astype(np.float32), flip.astype(np.uint8), present.astype(np.int32))]
    rg = upload(np.asarray(rows, np.int32)) if rows is not None else None
    _lib.check(lib.pn_explain_totals(ctx, S, G, ins[0].ptr(), ins[1].ptr(), ins[2].ptr(), ins[3].ptr(),
                                     rg.ptr() if rg is not None else None, len(rows) if rows is not None else 0, tot.ptr(), stream))
    torch.cuda.synchronize()
    assert all(g.intact() for g in ins) and tot.intact() and (rg is None or rg.intact())


def read_totals(tot, G):
    raw = tot.payload.cpu().numpy()
    i = raw[:24 * G].view(np.int64).reshape(3, G)
    f = raw[24 * G:].view(np.float64).reshape(2, G)
    return ref.Totals(i[0].copy(), i[1].copy(), i[2].copy(), f[0].copy(), f[1].copy())


def test_totals():
    """exact integers, fp64 sums inside the bound; two calls of half the rows equal the restatement of the same sequence bit for
    bit; the rows subset with repeats and entries outside [0, S)"""
    S, G = 700, 5                   # three batches of 256 rows
    case = ref.make_case(S=S, W=5, H=8, C=3, G=G, seed=31)
    got, _ = gpu_groups(case)
    dd, kg, flip, present = got["drop_delta"].copy(), got["keep_gain"].copy(), got["flip"], got["present"]
    dd[5, 1], kg[300, 2] = np.nan, np.inf                   # rows left out of one group
    one = Guarded(40 * G, fill=0)
    gpu_totals(one, dd, kg, flip, present)
    t1 = read_totals(one, G)
    want, hi = ref.totals_add(ref.new_totals(G), dd, kg, flip, present), ref.new_totals(G, np.longdouble)
    ref.totals_add(hi, dd, kg, flip, present)
    ok = (present > 0) & np.isfinite(dd) & np.isfinite(kg)
    for k in ("rows_present", "members", "flips"):
        assert (getattr(t1, k) == getattr(want, k)).all(), k
    assert t1.rows_present.sum() > 0 and (t1.rows_present < S).any()
    for k, v in (("drop_delta_sum", dd), ("keep_gain_sum", kg)):
        assert (getattr(t1, k) == getattr(want, k)).all(), k            # the same ascending fp64 sum: the same bits
        bound = ref.tol_totals(np.where(ok, np.abs(v), 0).sum(0), S)
        assert (np.abs(getattr(t1, k) - getattr(hi, k)).astype(np.float64) <= bound).all(), k
    two, seq = Guarded(40 * G, fill=0), ref.new_totals(G)
    for rows in (np.arange(0, 350), np.arange(350, S)):
        gpu_totals(two, dd, kg, flip, present, rows=rows)
        ref.totals_add(seq, dd, kg, flip, present, rows=rows)
    t2 = read_totals(two, G)
    for k in ref.Totals._fields:
        assert (getattr(t2, k) == getattr(seq, k)).all(), k
    rows = np.array([3, 3, -1, S, 699, 9], np.int32)
    sub, want = Guarded(40 * G, fill=0), ref.totals_add(ref.new_totals(G), dd, kg, flip, present, rows=rows)
    gpu_totals(sub, dd, kg, flip, present, rows=rows)
    t3 = read_totals(sub, G)
    for k in ref.Totals._fields:
        assert (getattr(t3, k) == getattr(want, k)).all(), k
