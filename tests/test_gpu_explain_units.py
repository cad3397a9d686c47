"""pn_explain_units / pn_explain_overlap / pn_explain_node_totals on the GPU, through the C ABI, against the NumPy restatement
tests/explain_units_ref.py.

Every buffer sits between two guard bands of 0xFF bytes that must come back untouched, and outputs start as 0xFF themselves
(test_gpu_ensemble.Guarded).  Held to: unit, count, label, present, flip, target_used, status and the node table exactly --
the overlap inputs are drawn so that no two logits an argmax compares are closer than 1e-5 in the reference itself -- and
every fp32 output within ONE fp32 ulp of the long-double reference rounded to fp32 plus explain_ref's fp64 bound of the
partition call that removes the same members (explain_units_ref's docstring).  With one label per member the outputs are
pn_explain_groups' bits.
"""
import ctypes

import numpy as np
import pytest
import torch

import explain_ref as ref
import explain_units_ref as uref
from test_gpu_ensemble import Guarded, lib_ctx
from test_gpu_explain_kernel import ALL_OUT, DTYPES, F32_OUT, gpu_groups, upload

pytestmark = pytest.mark.gpu
BIG = 2 ** 31 - 1


# ---- pn_explain_units ------------------------------------------------------------------------------------------------------
def gpu_units(node, kind, exclude=None):
    """-> (unit [S, W * M], count [S], label [S, W, M]); guard bands checked"""
    _lib, lib, ctx, stream = lib_ctx()
    S, W, L = node.shape
    M = L - 1 if kind == uref.UNIT_EDGE else L
    src = upload(node.astype(np.int32))
    exc = upload(np.asarray(exclude, np.int32)) if exclude is not None else None
    unit, count, label = Guarded(8 * S * W * M), Guarded(4 * S), Guarded(4 * S * W * M)
    _lib.check(lib.pn_explain_units(ctx, S, W, L, kind, src.ptr(), exc.ptr() if exc else None, unit.ptr(), count.ptr(),
                                    label.ptr(), stream))
    torch.cuda.synchronize()
    for g in (src, unit, count, label) + ((exc,) if exc else ()):
        assert g.intact()
    if S == 0:
        assert unit.untouched() and count.untouched() and label.untouched()
    return unit.numpy(np.int64, (S, W * M)), count.numpy(np.int32, (S,)), label.numpy(np.int32, (S, W, M))


def draw_nodes(rng, S, W, L, span):
    """ids from a small range (repeats), with negatives and ids at 2^31 - 1; row 0 all equal, row 1 (if any) all distinct"""
    node = rng.integers(0, span, (S, W, L)).astype(np.int64)
    node[rng.random((S, W, L)) < 0.1] = -1
    node[rng.random((S, W, L)) < 0.05] = -7
    node[rng.random((S, W, L)) < 0.1] = BIG
    node[rng.random((S, W, L)) < 0.05] = BIG - 1
    if S > 0:
        node[0] = 5
    if S > 1:
        node[1] = BIG - rng.permutation(W * L).reshape(W, L)
    return node.astype(np.int32)


UNIT_SHAPES = [(n, 1) for n in (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024)] + [(64, 16), (5, 4), (40, 4), (3, 16)]
EDGE_SHAPES = [(n, 2) for n in (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024)] + [(68, 16), (5, 4), (341, 4), (40, 4)]


@pytest.mark.parametrize("kind,W,L", [(uref.UNIT_NODE, W, L) for W, L in UNIT_SHAPES]
                         + [(uref.UNIT_EDGE, W, L) for W, L in EDGE_SHAPES])
def test_units_over_the_key_counts(kind, W, L):
    """W * M on both sides of every wave, workgroup and power-of-two boundary up to the cap of 1024: a row of all-equal keys, a
    row of all-distinct keys, an entirely excluded row, negative ids and ids at 2^31 - 1; a second run leaves the same bits"""
    rng = np.random.default_rng(W * 31 + L)
    S = 4
    node = draw_nodes(rng, S, W, L, span=max(3, W // 2))
    exclude = None
    if kind == uref.UNIT_NODE:
        exclude = np.array([5, -1, node[2, 0, 0], node[3, -1, -1]], np.int32)      # row 0: every step is the excluded node
    got = gpu_units(node, kind, exclude)
    want = uref.units(node, kind, exclude)
    for g, w, name in zip(got, want, ("unit", "count", "label")):
        assert g.dtype == w.dtype and (g == w).all(), name
    M = L - 1 if kind == uref.UNIT_EDGE else L
    if kind == uref.UNIT_NODE:
        assert got[1][0] == 0 and (got[2][0] == -1).all() and (got[0][0] == -1).all()
    else:
        assert got[1][0] == 1 and (got[2][0] == 0).all() and got[0][0, 0] == uref.edge_key(5, 5)
    assert got[1][1] == W * M                                   # all distinct: the row is full
    again = gpu_units(node, kind, exclude)
    for g, a in zip(got, again):
        assert g.tobytes() == a.tobytes()


@pytest.mark.parametrize("kind", (uref.UNIT_NODE, uref.UNIT_EDGE))
@pytest.mark.parametrize("S", (0, 1, 3, 513))
def test_units_over_the_row_counts_and_split_calls(kind, S):
    """a row's tables are a function of the row alone: S = 513 (every CU takes a second row) equals the rows taken in two calls"""
    rng = np.random.default_rng(S + 7)
    W, L = 7, 5
    node = draw_nodes(rng, S, W, L, span=12)
    exclude = rng.integers(0, 12, S).astype(np.int32) if kind == uref.UNIT_NODE else None
    got = gpu_units(node, kind, exclude)
    want = uref.units(node, kind, exclude)
    for g, w, name in zip(got, want, ("unit", "count", "label")):
        assert (g == w).all(), name
    if S >= 3:
        cut = S // 3
        a = gpu_units(node[:cut], kind, None if exclude is None else exclude[:cut])
        b = gpu_units(node[cut:], kind, None if exclude is None else exclude[cut:])
        for g, x, y in zip(got, a, b):
            assert np.concatenate([x, y]).tobytes() == g.tobytes()
    if kind == uref.UNIT_NODE and S:
        free = gpu_units(node, kind, None)                       # exclude = NULL
        assert all((g == w).all() for g, w in zip(free, uref.units(node, kind)))


def test_units_argument_refusals():
    _lib, lib, ctx, stream = lib_ctx()
    buf = Guarded(1 << 16)

    def call(S=1, W=2, L=3, kind=uref.UNIT_NODE, node=buf.ptr(), exclude=None, unit=buf.ptr(), count=buf.ptr(), label=buf.ptr()):
        return lib.pn_explain_units(ctx, S, W, L, kind, node, exclude, unit, count, label, stream)
    for kw in (dict(S=-1), dict(S=2 ** 31), dict(W=0), dict(L=0), dict(L=17), dict(W=1025, L=1), dict(W=65, L=16),
               dict(kind=2), dict(kind=-1), dict(kind=uref.UNIT_EDGE, L=1), dict(kind=uref.UNIT_EDGE, W=1025, L=2),
               dict(kind=uref.UNIT_EDGE, W=69, L=16), dict(kind=uref.UNIT_EDGE, exclude=buf.ptr()), dict(node=None),
               dict(unit=None), dict(count=None), dict(label=None)):
        assert call(**kw) == _lib.PN_ERR_ARG, kw
    assert call(S=0, node=None, unit=None, count=None, label=None) == 0          # S == 0: nothing is read, nothing launched
    torch.cuda.synchronize()
    assert buf.untouched()


# ---- pn_explain_overlap ----------------------------------------------------------------------------------------------------
def gpu_overlap(case, want=ALL_OUT, rows=None, with_status=True):
    """-> ({name: numpy}, status [2] or None).  rows: a slice of the case's rows"""
    _lib, lib, ctx, stream = lib_ctx()
    sl = slice(None) if rows is None else rows
    state, coef, ego, label = case.state[sl], case.coef[sl], case.ego[sl], case.label[sl]
    weight = None if case.weight is None else case.weight[sl]
    target = None if case.target is None else case.target[sl]
    S, W, H = state.shape
    C, G, M = case.fc2_w.shape[0], case.G, case.M
    assert label.shape == (S, W, M)
    ins = dict(state=upload(state), coef=upload(coef), ego=upload(ego), fc2_w=upload(case.fc2_w), fc2_b=upload(case.fc2_b),
               label=upload(label.astype(np.int32)))
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
    _lib.check(lib.pn_explain_overlap(ctx, S, W, H, C, G, M, p("state"), H, p("coef"), p("ego"), H, p("fc2_w"), 2 * H,
                                      p("fc2_b"), p("weight"), p("label"), case.norm, case.renorm, p("target"),
                                      ctypes.byref(out), status.ptr() if status else None, stream))
    torch.cuda.synchronize()
    for k, g in list(ins.items()) + list(bufs.items()):
        assert g.intact(), k
    got = {k: g.numpy(DTYPES.get(k, np.float32), shapes[k]) for k, g in bufs.items()}
    st = None
    if status is not None:
        assert status.intact()
        st = status.numpy(np.int32, (2,))
    return got, st


def check(got, st, case, tag=""):
    """every output against the long-double restatement; -> the fp64 restatement"""
    lo, hi = uref.run(case), uref.run(case, np.longdouble)
    if case.fc2_w.shape[0] > 1:
        assert ref.min_gap(lo) >= uref.GAP, "the case holds logits closer than 1e-5: choose another seed"
    for k in ("flip", "present", "target_used"):
        if k in got:
            assert (got[k] == getattr(lo, k)).all(), k
    if st is not None:
        assert st.tolist() == lo.status.tolist()
    worst = {}
    for k in F32_OUT:
        if k not in got:
            continue
        want = ref.f32(getattr(hi, k))
        tol = ref.ulp32(want) + hi.tol[k]
        nan = np.isnan(want)
        assert (np.isnan(got[k]) == nan).all(), k
        err = np.abs(got[k].astype(np.float64) - want.astype(np.float64))
        err[nan] = 0
        worst[k] = float((err / np.where(nan, 1, tol)).max()) if err.size else 0.0
        assert (err <= np.where(nan, 1, tol)).all(), "%s off by %g of its tolerance" % (k, worst[k])
    print("explain-overlap-error %s: worst error / tolerance %s" % (tag, {k: round(v, 3) for k, v in worst.items()}))
    return lo


AXES = [dict(ref.BASE, H=33), dict(ref.BASE, W=65), dict(ref.BASE, C=17), dict(ref.BASE, G=70), dict(ref.BASE, S=513)]


@pytest.mark.parametrize("sh", AXES, ids=lambda sh: "-".join("%s%d" % kv for kv in sh.items()))
def test_one_label_per_member_has_pn_explain_groups_bits(sh):
    """M = 1 and label = group on five rows of explain_ref.shape_table(), one per axis: every output, bit for bit"""
    idx = ref.shape_table().index(sh)
    part = ref.make_case(seed=100 + idx, renorm=idx % 2, norm=(idx // 2) % 2, **sh)
    want, st_want = gpu_groups(part)
    case = uref.Case(*part[:6], part.group[:, :, None], part.G, 1, part.norm, part.renorm, part.target)
    got, st = gpu_overlap(case)
    for k in ALL_OUT:
        assert got[k].tobytes() == want[k].tobytes(), k
    assert st.tolist() == st_want.tolist()


@pytest.mark.parametrize("M", (2, 4, 16))
def test_overlapping_labels_at_the_base_shape(M):
    redraws = []
    case = uref.make_case(S=3, W=5, H=32, C=3, G=6, M=M, seed=40 + M, renorm=M % 4 == 0, redraws=redraws)
    assert redraws[0] <= 200
    assert (case.label == -1).any() and (case.label == 6).any()            # a label of -1 and a label of G: no membership
    got, st = gpu_overlap(case)
    lo = check(got, st, case, "base M=%d" % M)
    assert (lo.present.sum(1) > (np.isfinite(case.weight) & (case.weight > 0)).sum(1)).any()     # members in several groups
    again, _ = gpu_overlap(case)
    for k in ALL_OUT:
        assert got[k].tobytes() == again[k].tobytes(), k


@pytest.mark.parametrize("sh", [dict(S=2, W=64, H=32, C=3, G=1024, M=16),         # the cap: W * M = 1024, more than 64 KB of LDS
                                dict(S=2, W=40, H=128, C=7, G=160, M=4),         # the hot shape of groups="node"
                                dict(S=2, W=130, H=33, C=65, G=8, M=2)],         # chunked route: (W + 1) * C > 4096
                         ids=("cap", "hot", "chunked"))
def test_around_the_cap_the_hot_shape_and_the_chunked_route(sh):
    _lib, lib, _, _ = lib_ctx()
    route = (ctypes.c_int32 * 4)()
    _lib.check(lib.pn_explain_route(sh["S"], sh["W"], sh["H"], sh["C"], sh["G"], route))
    assert route[0] == (ref.ROUTE_CHUNKED if sh["C"] == 65 else ref.ROUTE_ROW)
    case = uref.make_case(seed=50, renorm=1, **sh)
    got, st = gpu_overlap(case)
    check(got, st, case, str(sh))
    if sh["M"] == 4:                # rows split over two calls leave the bits of one
        big = uref.make_case(seed=51, **dict(sh, S=5))
        whole, _ = gpu_overlap(big)
        a, _ = gpu_overlap(big, rows=slice(0, 2))
        b, _ = gpu_overlap(big, rows=slice(2, 5))
        for k in ALL_OUT:
            assert np.concatenate([a[k], b[k]]).tobytes() == whole[k].tobytes(), k


@pytest.mark.parametrize("norm", (ref.NORM_SUM, ref.NORM_COUNT))
@pytest.mark.parametrize("renorm", (0, 1))
def test_norms_weights_dead_members_and_a_hub(norm, renorm):
    """both norms x renorm, weights NULL against all ones (the same bits), dead members of every kind, a unit on every member
    (its drop is e: no live member remains), targets given, free and out of range"""
    sh = dict(S=9, W=7, H=33, C=5, G=6, M=3)
    case = uref.make_case(seed=61, norm=norm, renorm=renorm, weights=False, **sh)
    got, st = gpu_overlap(case)
    check(got, st, case, "unweighted")
    ones, _ = gpu_overlap(case._replace(weight=np.ones((9, 7), np.float32)))
    for k in ALL_OUT:
        assert got[k].tobytes() == ones[k].tobytes(), k
    dead = uref.make_case(seed=63, norm=norm, renorm=renorm, weights=True, hub=True, **sh)
    assert (~np.isfinite(dead.weight)).any() and (dead.weight == 0).any()
    got, st = gpu_overlap(dead, want=ALL_OUT)
    lo = check(got, st, dead, "dead members, hub")
    live = (np.isfinite(dead.weight) & (dead.weight > 0)).sum(1)
    assert (got["present"][:, 0] == live).all()                          # the hub: every live member, counted once
    e = ref.f32(lo.e)
    assert (np.abs(got["drop_logits"][:, 0] - e) <= ref.ulp32(e)).all()   # nothing remains: the logits are e
    free = dead._replace(target=None)
    got, st = gpu_overlap(free)
    lo = check(got, st, free, "free target")
    assert (got["target_used"] == lo.full.argmax(1)).all()
    tgt = dead.target.copy()
    tgt[[1, 4]] = (5, -3)
    off = dead._replace(target=tgt)
    got, st = gpu_overlap(off)
    check(got, st, off, "targets out of range")
    assert st.tolist() == [2, 0] and (got["drop_delta"][[1, 4]] == 0).all() and (got["flip"][[1, 4]] == 0).all()
    gpu_overlap(off, with_status=False)                                  # a NULL status is not written to


@pytest.mark.parametrize("where", ("state", "coef", "ego"))
def test_a_non_finite_entry_makes_exactly_that_row_bad(where):
    case = uref.make_case(S=6, W=5, H=32, C=3, G=6, M=3, seed=71)
    clean, _ = gpu_overlap(case)
    a = getattr(case, where).copy()
    a[(2, 4, 31) if where == "state" else (2, 4)] = {"state": np.inf, "coef": np.nan, "ego": -np.inf}[where]
    hurt = case._replace(**{where: a})
    got, st = gpu_overlap(hurt)
    check(got, st, hurt, "bad row")
    assert st.tolist() == [0, 1]
    keep = np.arange(6) != 2
    for k in ALL_OUT:
        assert got[k][keep].tobytes() == clean[k][keep].tobytes(), k
    for k in F32_OUT:
        assert np.isnan(got[k][2]).all(), k
    assert (got["flip"][2] == 0).all() and (got["present"][2] == clean["present"][2]).all()


def test_each_output_is_optional():
    case = uref.make_case(S=5, W=5, H=32, C=3, G=6, M=2, seed=72)
    whole, _ = gpu_overlap(case)
    for leave in ALL_OUT:
        got, _ = gpu_overlap(case, want=tuple(k for k in ALL_OUT if k != leave))
        for k in got:
            assert got[k].tobytes() == whole[k].tobytes(), (leave, k)
    got, _ = gpu_overlap(case, want=("drop_delta", "flip"))
    assert got["drop_delta"].tobytes() == whole["drop_delta"].tobytes() and (got["flip"] == whole["flip"]).all()
    gpu_overlap(case, want=())


def test_overlap_argument_refusals():
    _lib, lib, ctx, stream = lib_ctx()
    buf = Guarded(1 << 16)
    out = _lib.ExplainOut()

    def call(S=1, W=2, H=4, C=3, G=2, M=2, ld_state=4, ld_ego=4, ld_w=8, norm=0, renorm=0, state=buf.ptr(), label=buf.ptr(),
             out=ctypes.byref(out)):
        return lib.pn_explain_overlap(ctx, S, W, H, C, G, M, state, ld_state, buf.ptr(), buf.ptr(), ld_ego, buf.ptr(), ld_w,
                                      buf.ptr(), None, label, norm, renorm, None, out, None, stream)
    for kw in (dict(M=0), dict(M=17), dict(W=1025, M=1), dict(W=205, M=5), dict(W=65, M=16), dict(S=-1), dict(S=2 ** 31),
               dict(W=0), dict(G=0), dict(G=1025), dict(H=0), dict(H=4097), dict(C=0), dict(C=1025), dict(ld_state=3),
               dict(ld_ego=3), dict(ld_w=7), dict(norm=2), dict(renorm=2), dict(state=None), dict(label=None), dict(out=None)):
        assert call(**kw) == _lib.PN_ERR_ARG, kw
    assert call(S=0, state=None, label=None) == 0
    torch.cuda.synchronize()
    assert buf.untouched()


# ---- pn_explain_node_totals ------------------------------------------------------------------------------------------------
def gpu_node_totals(tab, N, unit, dd, kg, flip, present, rows=None):
    _lib, lib, ctx, stream = lib_ctx()
    S, G = dd.shape
    ins = [upload(a) for a in (unit.astype(np.int64), dd.astype(np.float32), kg.astype(np.float32), flip.astype(np.uint8),
                               present.astype(np.int32))]
    rg = upload(np.asarray(rows, np.int32)) if rows is not None else None
    _lib.check(lib.pn_explain_node_totals(ctx, S, G, N, *(g.ptr() for g in ins), rg.ptr() if rg is not None else None,
                                          len(rows) if rows is not None else 0, tab.ptr(), stream))
    torch.cuda.synchronize()
    assert all(g.intact() for g in ins) and tab.intact() and (rg is None or rg.intact())


def test_node_totals():
    """exact against the restatement: one call, two consecutive calls into one table, a rows list with repeats and entries
    outside [0, S), keys outside [0, N) (skipped, also as the row's best), non-finite scores, absent units"""
    rng = np.random.default_rng(81)
    S, W, L, N = 300, 6, 4, 50
    G = W * L
    node = rng.integers(0, 60, (S, W, L)).astype(np.int32)              # ids 50 .. 59 are outside the table
    unit, count, label = uref.units(node, uref.UNIT_NODE)
    dd = rng.standard_normal((S, G)).astype(np.float32)
    dd[:, 1] = dd[:, 0]                                                 # ties: the lower position is the row's best
    kg = rng.standard_normal((S, G)).astype(np.float32)
    dd[5, 1], kg[7, 2], dd[9, 0] = np.nan, np.inf, -np.inf
    flip = (rng.random((S, G)) < 0.3).astype(np.uint8)
    present = np.where(np.arange(G)[None, :] < count[:, None], rng.integers(0, 4, (S, G)), 0).astype(np.int32)
    args = (unit, dd, kg, flip, present)

    def read(tab):
        t = tab.numpy(np.int64, (4, N))
        return uref.NodeTable(t[0], t[1], t[2], t[3])
    one = Guarded(32 * N, fill=0)
    gpu_node_totals(one, N, *args)
    want = uref.node_totals_add(uref.new_table(N), *args)
    for k in uref.NodeTable._fields:
        assert (getattr(read(one), k) == getattr(want, k)).all(), k
    assert want.top.sum() > 0 and want.top.sum() <= S and want.flips.sum() > 0
    two, seq = Guarded(32 * N, fill=0), uref.new_table(N)
    for rows in (np.arange(0, 130), np.arange(130, S)):
        gpu_node_totals(two, N, *args, rows=rows)
        uref.node_totals_add(seq, *args, rows=rows)
    for k in uref.NodeTable._fields:
        assert (getattr(read(two), k) == getattr(seq, k)).all() and (getattr(seq, k) == getattr(want, k)).all(), k
    rows = np.array([3, 3, -1, S, 299, 9, 2 ** 31 - 1], np.int32)
    sub, want = Guarded(32 * N, fill=0), uref.node_totals_add(uref.new_table(N), *args, rows=rows)
    gpu_node_totals(sub, N, *args, rows=rows)
    for k in uref.NodeTable._fields:
        assert (getattr(read(sub), k) == getattr(want, k)).all(), k
    small = Guarded(32 * 7, fill=0)                                     # most keys outside [0, 7)
    gpu_node_totals(small, 7, *args)
    want = uref.node_totals_add(uref.new_table(7), *args)
    t = small.numpy(np.int64, (4, 7))
    assert (t == np.stack(want)).all()


def test_node_totals_argument_refusals():
    _lib, lib, ctx, stream = lib_ctx()
    buf = Guarded(4096)
    t = lambda **kw: lib.pn_explain_node_totals(ctx, kw.get("S", 1), kw.get("G", 2), kw.get("N", 5), kw.get("unit", buf.ptr()),   # noqa: E731
                                                kw.get("dd", buf.ptr()), buf.ptr(), buf.ptr(), buf.ptr(), kw.get("rows"),
                                                kw.get("n", 0), kw.get("tab", buf.ptr()), stream)
    for kw in (dict(S=-1), dict(G=0), dict(G=1025), dict(N=0), dict(n=3), dict(n=-1, rows=buf.ptr()), dict(unit=None),
               dict(dd=None), dict(tab=None)):
        assert t(**kw) == _lib.PN_ERR_ARG, kw
    assert t(S=0, unit=None, dd=None, tab=None) == 0 and t(rows=buf.ptr(), n=0, tab=None) == 0
    torch.cuda.synchronize()
    assert buf.untouched()
