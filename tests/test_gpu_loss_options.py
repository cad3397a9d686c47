"""Class weights, ignore_index and label smoothing of the training loss on the GPU: pn_cross_entropy_ex against the fp64
reference of tests/loss_ref.py within its bounds (as close to fp64 as stock fp32 torch, factor 8, floor 2e-6), the edge
behaviour the header states, the fused step (forward_loss(loss=...)) on every pooling route against the CPU oracle with
torch's loss and autograd, the routes against each other, a captured step whose ignored count changes between replays, and
the trainer."""
import ctypes
import math
import os

import loss_ref as R
import numpy as np
import pytest
import torch
from gradcheck import ZERO_OK_HETERO, assert_grads_close

from oracle import pagg_oracle as po

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
PAD = 64
U = 2.0 ** -24


def _guarded(n):
    """an fp32 buffer of n elements between two sentinel fences -> (whole, the n elements)"""
    whole = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    return whole, whole[PAD:PAD + n]


def _fences_intact(whole, n):
    return bool((whole[:PAD] == SENTINEL).all()) and bool((whole[PAD + n:] == SENTINEL).all())


def run_ex(x, t, w=None, ii=None, eps=0.0, reduction="mean", grad_scale=1.0, want_grad=True, given=None):
    """pn_cross_entropy_ex -> (loss, grad or None, D or None) on the CPU; loss, g_logits and the denominator sit between
    sentinel fences (nothing outside them may be written) and start as NaN (everything inside must be)"""
    from pathnet_amd import _lib
    lib = _lib.load()
    rows, C = x.shape
    xd, td = x.cuda().contiguous(), t.cuda().contiguous()
    wd = None if w is None else w.cuda().contiguous()
    lw, loss = _guarded(1)
    gw, g = _guarded(rows * C) if want_grad else (None, None)
    dw, den = _guarded(1)
    loss.fill_(float("nan"))
    if g is not None:
        g.fill_(float("nan"))
    den.fill_(float("nan") if given is None else float(given))
    mean = reduction == "mean"
    spec = _lib.LossSpec(_lib.ptr(wd), ii if ii is not None else 0, 0 if ii is None else 1, eps,
                         _lib.LOSS_MEAN if mean else _lib.LOSS_SUM, grad_scale, _lib.ptr(den), 0 if given is None else 1)
    _lib.check(lib.pn_cross_entropy_ex(_lib.ptr(xd), _lib.ptr(td), rows, C, ctypes.byref(spec), _lib.ptr(loss), _lib.ptr(g),
                                       _lib.stream_ptr(xd.device)))
    torch.cuda.synchronize()
    assert _fences_intact(lw, 1) and _fences_intact(dw, 1) and (gw is None or _fences_intact(gw, rows * C))
    return loss.item(), None if g is None else g.view(rows, C).cpu().double(), den.item()


def check_against_ref(x, t, w, ii, eps, reduction, tag, grad_scale=1.0):
    got_l, got_g, got_d = run_ex(x, t, w, ii, eps, reduction, grad_scale)
    ref = R.loss_ref(x, t, w, ii, eps, reduction, grad_scale)
    rows = x.shape[0]
    # D: thread i adds rows i, i + 1024, ... (ceil(rows / 1024) additions), then 6 + 4 levels of pairwise sums: each fp32
    # addition is charged u of the (non-negative) partial sum, so (ceil(rows / 1024) + 10) u D bounds it
    assert abs(got_d - ref["D"]) <= (math.ceil(rows / 1024) + 10) * U * ref["D"], (tag, got_d, ref["D"])
    assert torch.isfinite(got_g).all(), tag
    if reduction == "mean" and ref["D"] == 0.0:         # the library's rule: NaN loss, zero gradients
        assert math.isnan(got_l) and (got_g == 0).all(), (tag, got_l)
        return
    lb, gb = R.loss_bounds(ref)
    lerr, gerr = abs(got_l - ref["loss"]), (got_g - ref["grad"]).abs().max().item()
    print("%s: loss err %.3g (bound %.3g), grad err %.3g (bound %.3g)" % (tag, lerr, lb, gerr, gb))
    assert lerr <= lb, (tag, got_l, ref["loss"], lb)
    assert gerr <= gb, (tag, gerr, gb)
    if ii is not None:
        assert (got_g[t == ii] == 0).all(), tag


@pytest.mark.parametrize("rows", R.GPU_ROWS)
def test_ex_kernel_rows_around_the_one_workgroup_line(rows):
    for name, (weights, ignore, eps, reduction) in R.GPU_OPTIONS.items():
        x, t, w, ii = R.make_case(rows, 3, weights, ignore, seed=1)
        check_against_ref(x, t, w, ii, eps, reduction, "rows %d %s" % (rows, name))


@pytest.mark.parametrize("C", R.GPU_CLASSES)
def test_ex_kernel_class_counts(C):
    for name, (weights, ignore, eps, reduction) in R.GPU_OPTIONS.items():
        x, t, w, ii = R.make_case(33, C, weights, ignore, seed=2)
        check_against_ref(x, t, w, ii, eps, reduction, "C %d %s" % (C, name), grad_scale=2.5 if name == "all" else 1.0)


def test_ex_kernel_without_gradient_and_with_every_option_off():
    from pathnet_amd import _lib
    lib = _lib.load()
    x, t, w, ii = R.make_case(65, 7, "zero", -1, seed=3)
    l0, g0, d0 = run_ex(x, t, w, ii, 0.1, "mean")
    l1, g1, d1 = run_ex(x, t, w, ii, 0.1, "mean", want_grad=False)             # g_logits = NULL
    assert g1 is None and l0 == l1 and d0 == d1
    # all options off: pn_cross_entropy's bits (the loss where one workgroup stores it; past that both add their parts with
    # atomics, whose order is free -- the gradient is row-wise and has the same bits at any row count)
    for rows in (1, 65, 1025, 32768, 32769):
        x, t, _, _ = R.make_case(rows, 3, "none", "none", seed=4)
        xd, td = x.cuda(), t.cuda()
        loss = torch.empty((), device="cuda")
        g = torch.empty_like(xd)
        _lib.check(lib.pn_cross_entropy(_lib.ptr(xd), _lib.ptr(td), rows, 3, _lib.ptr(loss), _lib.ptr(g),
                                        _lib.stream_ptr(xd.device)))
        le, ge, de = run_ex(x, t)
        assert torch.equal(ge.float(), g.cpu()), rows
        assert de == rows
        if rows <= 32768:
            assert le == loss.item(), rows
        else:
            # (ceil(rows / 256) workgroups add their parts to the loss with atomics in whatever order they finish -- the plain
            #  call does not repeat its own last bits here: each of the blocks - 1 additions rounds by at most u |loss|
            #  (the parts are non-negative), so two orders lie within 2 (blocks - 1) u |loss| of each other)
            blocks = min(-(-rows // 256), 256)
            assert abs(le - loss.item()) <= 2 * (blocks - 1) * U * abs(le), rows


def test_python_cross_entropy_takes_the_options_and_keeps_the_plain_call():
    from pathnet_amd import optim
    x, t, w, ii = R.make_case(33, 7, "random", -100, seed=5)
    xd = x.cuda().requires_grad_(True)
    loss = optim.cross_entropy(xd, t.cuda(), weight=w.cuda(), ignore_index=ii, label_smoothing=0.1)
    (3.0 * loss).backward()
    ref = R.loss_ref(x, t, w, ii, 0.1, "mean")
    lb, gb = R.loss_bounds(ref)
    assert abs(loss.item() - ref["loss"]) <= lb
    assert (xd.grad.cpu().double() - 3.0 * ref["grad"]).abs().max().item() <= 3.0 * gb + 3 * U * ref["grad"].abs().max().item()
    mod = optim.CrossEntropyLoss(weight=w, ignore_index=ii, label_smoothing=0.1).cuda()
    assert mod(x.cuda(), t.cuda()).item() == loss.item()
    s = optim.cross_entropy(x.cuda(), t.cuda(), reduction="sum", ignore_index=ii)
    assert abs(s.item() - R.loss_ref(x, t, None, ii, 0.0, "sum")["loss"]) <= 1e-5 * abs(s.item())
    # defaults: the old entry point, and -1 still poisons the loss
    x2, t2, _, _ = R.make_case(33, 7, "none", "none", seed=6)
    assert optim.cross_entropy(x2.cuda(), t2.cuda()).item() == optim.CrossEntropyLoss()(x2.cuda(), t2.cuda()).item()
    t2[3] = -1
    assert math.isnan(optim.CrossEntropyLoss()(x2.cuda(), t2.cuda()).item())
    assert math.isfinite(optim.CrossEntropyLoss(ignore_index=-1)(x2.cuda(), t2.cuda()).item())
    with pytest.raises(ValueError):
        optim.CrossEntropyLoss(weight=torch.ones(5))(x2.cuda(), t2.cuda())
    # balanced weights on the device, nothing read back
    wb = optim.balanced_class_weight(t.cuda(), 7, ignore_index=ii)
    assert wb.is_cuda and torch.allclose(wb.cpu(), optim.balanced_class_weight(t, 7, ignore_index=ii))


def test_edge_behaviour():
    x, t, w, _ = R.make_case(70, 5, "random", "none", seed=7)
    # ignored rows: exact zero gradient rows, and their logits may be NaN without touching the loss or the other rows
    ti = t.clone()
    ti[::4] = -1
    l0, g0, d0 = run_ex(x, ti, w, -1, 0.1)
    xn = x.clone()
    xn[::4] = float("nan")
    l1, g1, d1 = run_ex(xn, ti, w, -1, 0.1)
    assert (g0[::4] == 0).all() and l0 == l1 and d0 == d1 and torch.equal(g0, g1) and math.isfinite(l0)
    # an out-of-range target that is not the ignore value: NaN loss, a zero row, the other rows right (D without it)
    tb = ti.clone()
    tb[1], tb[2] = 5, -2
    lb_, gb_, db_ = run_ex(x, tb, w, -1, 0.1)
    ref = R.loss_ref(x, tb, w, -1, 0.1)
    good = torch.ones(70, dtype=torch.bool)
    good[1] = good[2] = False
    sub = R.loss_ref(x[good], tb[good], w, -1, 0.1)
    assert math.isnan(lb_) and (gb_[1] == 0).all() and (gb_[2] == 0).all()
    assert abs(db_ - ref["D"]) <= 11 * U * ref["D"]
    assert (gb_[good] - sub["grad"]).abs().max().item() <= R.loss_bounds(sub)[1]
    # every row ignored: NaN loss, all-zero gradients, D = 0; the sum is a plain zero
    la, ga, da = run_ex(x, torch.full_like(t, -100), w, -100, 0.1)
    assert math.isnan(la) and (ga == 0).all() and da == 0.0
    ls, gs, _ = run_ex(x, torch.full_like(t, -100), w, -100, 0.1, "sum")
    assert ls == 0.0 and (gs == 0).all()
    # only zero-weight classes among the kept rows: the same (torch: NaN gradients)
    w0 = w.clone()
    w0[2] = 0.0
    lz, gz, dz = run_ex(x, torch.full_like(t, 2), w0)
    assert math.isnan(lz) and (gz == 0).all() and dz == 0.0
    # an ignore_index that is a valid class id drops that class's rows
    lc, gc, dc = run_ex(x, t, w, 3, 0.0)
    refc = R.loss_ref(x, t, w, 3, 0.0)
    assert (t == 3).any() and (gc[t == 3] == 0).all() and abs(lc - refc["loss"]) <= R.loss_bounds(refc)[0]
    assert abs(dc - refc["D"]) <= 11 * U * refc["D"]
    # denominator_given: a D other than the call's own scales loss and gradients by exactly that, and is left as given
    lg, gg, dg = run_ex(x, ti, w, -1, 0.1, given=2.0 * d0)
    assert dg == 2.0 * d0 and lg == l0 / 2.0 and torch.equal(gg, g0 / 2.0)
    refg = R.loss_ref(x, ti, w, -1, 0.1, denominator=3.5)
    l35, g35, _ = run_ex(x, ti, w, -1, 0.1, given=3.5)
    assert abs(l35 - refg["loss"]) <= 4e-6 * abs(refg["loss"])
    assert (g35 - refg["grad"]).abs().max().item() <= 4e-6 * refg["grad"].abs().max().item()


def test_denominator_entry_point():
    from pathnet_amd import _lib
    lib = _lib.load()
    for rows in (1, 1025, 40000):
        _, t, w, ii = R.make_case(rows, 9, "zero", -1, seed=8)
        t[0] = 11                               # no class: adds nothing
        td, wd = t.cuda(), w.cuda()
        dw, den = _guarded(1)
        spec = _lib.LossSpec(_lib.ptr(wd), ii, 1, 0.0, _lib.LOSS_SUM, 1.0, _lib.ptr(den), 1)
        runs = []
        for _ in range(2):
            den.fill_(float("nan"))
            _lib.check(lib.pn_loss_denominator(_lib.ptr(td), rows, 9, ctypes.byref(spec), _lib.stream_ptr(td.device)))
            torch.cuda.synchronize()
            runs.append(den.item())
        kept = (t >= 0) & (t < 9)
        want = w.double()[t[kept]].sum().item()
        assert runs[0] == runs[1] and _fences_intact(dw, 1)         # a fixed order: the same bits
        assert abs(runs[0] - want) <= (math.ceil(rows / 1024) + 10) * U * max(want, 1e-30), (rows, runs[0], want)


# ---- the fused step ---------------------------------------------------------------------------------------------------
N, F, S = 300, 24, 37


def _module(variant, H, C, L, seed=0):
    import pathnet_amd
    torch.manual_seed(seed)
    cls = {"homo": pathnet_amd.PathNet_homo, "hetero": pathnet_amd.PathNet, "pagg": pathnet_amd.PAGG}[variant]
    m = cls(F, H, C, L if variant != "pagg" else N).cuda().eval()       # (eval: no dropout; forward_loss needs grad mode only)
    with torch.no_grad():
        for k, v in m.named_parameters():
            if k.endswith("bias") or "bias_" in k:
                v.uniform_(-0.3, 0.3)
    return m


def _batch(W, L, C, seed=0, s=S, ignored=None):
    """X, ids, codes, sel, targets with -1 on about a third of the rows (or exactly on `ignored`), class weights with a zero"""
    g = torch.Generator().manual_seed(100 + seed)
    X = torch.rand(N, F, generator=g)
    sel = torch.randperm(N, generator=g)[:s].sort().values
    ids = torch.randint(0, N, (s, W, L), generator=g).to(torch.int32)
    ids[:, :, 0] = sel[:, None].to(torch.int32)
    codes = torch.randint(0, L, (s, W, L), generator=g).to(torch.uint8)
    y = torch.randint(0, C, (s,), generator=g)
    if ignored is None:
        y[torch.rand(s, generator=g) < 1.0 / 3.0] = -1
    else:
        y[ignored] = -1
    w = torch.rand(C, generator=g) * 2.0 + 0.25
    w[C // 3] = 0.0
    return X, ids, codes, sel, y, w


def _step(m, batch, loss_fn, fused, grad_scale=None, upstream=1.0):
    X, ids, codes, sel, y, _ = batch
    m.zero_grad(set_to_none=True)
    W, L = ids.shape[1], ids.shape[2]
    loss, out = m.forward_loss(X.cuda(), ids.cuda(), W, L, sel.to(torch.int32).cuda(), codes.cuda(), y.cuda(), fused=fused,
                               loss=loss_fn, grad_scale=grad_scale)
    (loss * upstream if upstream != 1.0 else loss).backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), out.detach().cpu(), {k: v.grad.detach().cpu().clone() for k, v in m.named_parameters()}


def _oracle(m, variant, batch, eps, reduction="mean", factor=1.0):
    X, ids, codes, sel, y, w = batch
    W, L = ids.shape[1], ids.shape[2]
    params = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    want = po.forward(variant, params, X, ids.numpy(), codes.numpy(), sel.numpy(), W, L)
    wl = torch.nn.functional.cross_entropy(want, y, weight=w, ignore_index=-1, label_smoothing=eps, reduction=reduction)
    (factor * wl).backward()
    return wl.detach(), want.detach(), {k: params[k].grad for k, _ in m.named_parameters()}


def _loss_fn(batch, eps=0.1, reduction="mean"):
    from pathnet_amd import optim
    return optim.CrossEntropyLoss(weight=batch[5], ignore_index=-1, label_smoothing=eps, reduction=reduction).cuda()


def _check_fused(variant, W, H, C, L=3, knob=None, det=False, sparse=False, budget_groups=0, ignored=None, tag=""):
    from pathnet_amd import _lib
    from pathnet_amd import modules as M
    if variant == "pagg":
        L = 4           # (the class has its four distance layers: the one walk length it takes)
    m = _module(variant, H, C, L)
    m.deterministic = det
    if sparse:
        m.sparse_features = "always"
    batch = _batch(W, L, C, ignored=ignored)
    if budget_groups:
        Hk = -(-H // 32) * 32
        kw = dict(cell=m._cell_kind, deterministic=det)
        m.workspace_budget = M.workspace_bytes(variant, N, F, Hk, C, S, W, L, batch_groups=budget_groups, **kw)
        assert M.pick_batch_groups(variant, N, F, Hk, C, S, W, L, m.workspace_budget, **kw) == budget_groups
    old = _lib.set_knob("PN_POOL_STEP", knob) if knob is not None else None
    try:
        loss, out, grads = _step(m, batch, _loss_fn(batch), True)
    finally:
        if old is not None:
            _lib.set_knob("PN_POOL_STEP", old)
    if sparse:
        assert m.fc0_route == "sparse"
    wl, want, wg = _oracle(m, variant, batch, 0.1)
    oerr, lerr = (out - want).abs().max().item(), abs(loss.item() - wl.item())
    print("%s: logits err %.3g, loss %.6f vs %.6f (err %.3g)" % (tag, oerr, loss.item(), wl.item(), lerr))
    assert oerr < 1e-5 * max(1.0, want.abs().max().item())
    assert lerr < 1e-5 * max(1.0, abs(wl.item()))
    assert_grads_close(grads, wg, zero_ok=ZERO_OK_HETERO if variant == "hetero" else ())
    return m, batch, loss, grads


@pytest.mark.parametrize("H,C", [(32, 5), (128, 5), (32, 70), (128, 70)])
def test_fused_step_pool_step2_against_the_oracle(H, C):
    """pool_step2_loss_kernel: W = 5 gives wave 0 a second member, C = 70 makes the lane-per-class loops run twice"""
    _check_fused("homo", 5, H, C, tag="pool_step2 H %d C %d" % (H, C))


@pytest.mark.parametrize("W,H,knob,det", [
    (41, 128, None, False),     # pool_step_loss_kernel<4>: more members than pool_step2 holds
    (5, 160, None, False),      # pool_step_loss_kernel<4>: a hidden size past pool_step2's
    (5, 512, None, False),      # pool_step_loss_kernel<16>
    (5, 128, 2, False),         # PN_POOL_STEP = 2: the three bodies in one launch
    (5, 128, 0, False),         # PN_POOL_STEP = 0: the three launches
    (5, 128, None, True),       # deterministic mode: the three launches, fixed-order scatters
])
def test_fused_step_other_routes_against_the_oracle(W, H, knob, det):
    _check_fused("homo", W, H, 5, knob=knob, det=det, tag="W %d H %d knob %s det %s" % (W, H, knob, det))


@pytest.mark.parametrize("variant", ["hetero", "homo", "pagg"])
def test_fused_step_variants_with_sparse_features(variant):
    _check_fused(variant, 5, 64, 5, sparse=True, tag=variant + " sparse")


@pytest.mark.parametrize("det", [False, True])
def test_fused_step_in_micro_batches_divides_by_the_whole_call_s_denominator(det):
    """batch_groups = 16: 37 rows run as 16 + 16 + 5; every row of the second micro-batch is ignored, and D is the whole
    call's -- a per-micro-batch denominator would be 0 there and off everywhere else"""
    ignored = torch.zeros(S, dtype=torch.bool)
    ignored[16:32] = True
    ignored[3] = ignored[34] = True
    _check_fused("homo", 5, 64, 5, det=det, budget_groups=16, ignored=ignored, tag="micro det %s" % det)


def test_routes_agree_and_the_deterministic_mode_is_bitwise():
    from pathnet_amd import _lib, optim
    m = _module("homo", 128, 5, 3)
    batch = _batch(5, 3, 5)
    fn = _loss_fn(batch)
    # deterministic mode: fused and three calls run the same kernels -- bitwise, twice over
    m.deterministic = True
    l0, o0, g0 = _step(m, batch, fn, False)
    l1, o1, g1 = _step(m, batch, fn, True)
    l2, o2, g2 = _step(m, batch, fn, True)
    assert torch.equal(o0, o1) and l0.item() == l1.item() == l2.item()
    for k in g0:
        assert torch.equal(g0[k], g1[k]) and torch.equal(g1[k], g2[k]), k
    # default mode: the three launches and the one launch of the same bodies give the three calls' logits and loss bit for
    # bit, pool_step2 sums in another order (2e-6); gradients up to the order of the float atomics
    m.deterministic = False
    old = _lib.set_knob("PN_POOL_STEP", 0)
    try:
        la, oa, ga = _step(m, batch, fn, False)
        lb, ob, gb = _step(m, batch, fn, True)
        _lib.set_knob("PN_POOL_STEP", 2)
        lc, oc, gc = _step(m, batch, fn, True)
        _lib.set_knob("PN_POOL_STEP", 1)
        ld, od, gd = _step(m, batch, fn, True)
    finally:
        _lib.set_knob("PN_POOL_STEP", old)
    assert torch.equal(oa, ob) and torch.equal(ob, oc) and la.item() == lb.item() == lc.item()
    assert (od - oa).abs().max().item() <= 2e-6 * max(1.0, oa.abs().max().item())
    assert abs(ld.item() - la.item()) <= 2e-6 * max(1.0, abs(la.item()))
    for g in (gb, gc, gd):
        assert_grads_close(g, ga, rel=1e-5, noise=3e-8)
    # grad_scale multiplies as before, on either route; the upstream gradient scales the handed-out gradients
    m.deterministic = True
    ls, _, gs = _step(m, batch, fn, True, grad_scale=3.0 / S, upstream=0.5)
    lt, _, gt = _step(m, batch, fn, False, grad_scale=3.0 / S, upstream=0.5)
    assert abs(ls.item() - 3.0 * l1.item()) <= 4 * U * abs(ls.item()) and abs(lt.item() - ls.item()) <= 4 * U * abs(ls.item())
    assert_grads_close(gs, {k: 1.5 * v for k, v in g1.items()}, rel=1e-6)
    assert_grads_close(gt, gs, rel=1e-6)
    # loss=None and a loss without options: today's call, bit for bit
    lp, op, gp = _step(m, batch[:4] + (batch[4].clamp_min(0), batch[5]), None, True)
    lq, oq, gq = _step(m, batch[:4] + (batch[4].clamp_min(0), batch[5]), optim.CrossEntropyLoss(), True)
    assert lp.item() == lq.item() and torch.equal(op, oq) and all(torch.equal(gp[k], gq[k]) for k in gp)
    # ... and the sum reduction against the oracle's
    lsum, _, gsum = _step(m, batch, _loss_fn(batch, 0.1, "sum"), True)
    wl, _, wg = _oracle(m, "homo", batch, 0.1, "sum")
    assert abs(lsum.item() - wl.item()) < 1e-5 * abs(wl.item())
    assert_grads_close(gsum, wg)


def test_captured_step_follows_the_ignored_count_of_its_targets():
    """One fused step with ignore_index = -1 captured in a hipGraph (dropout seed from a StepState, as a captured training
    step has it) and replayed with three target tensors whose ignored counts differ: D is formed on the device by the
    replay, so each replay's loss is the eager call's on the same targets."""
    import pathnet_amd
    C, W, L, H = 4, 6, 3, 64
    X, ids, codes, sel, y, w = _batch(W, L, C, seed=9)
    torch.manual_seed(11)
    m = pathnet_amd.PathNet_homo(F, H, C, L, dropout=0.5).cuda().train()
    st = pathnet_amd.StepState("cuda", seed=77, first_epoch=0)
    st.advance()
    m.step_state = st
    fn = pathnet_amd.CrossEntropyLoss(weight=w, ignore_index=-1, label_smoothing=0.1).cuda()
    Xd, idsd, codesd, seld = X.cuda(), ids.cuda(), codes.cuda(), sel.to(torch.int32).cuda()
    tgt = y.clamp_min(0).cuda()
    loss_out = torch.zeros((), device="cuda")

    def step():
        loss, _ = m.forward_loss(Xd, idsd, W, L, seld, codesd, tgt, fused=True, loss=fn)
        loss_out.copy_(loss.detach())

    targets = []
    for count in (0, 9, 30):
        t = y.clamp_min(0).clone()
        t[:count] = -1
        targets.append(t.cuda())
    eager = []
    for t in targets:
        tgt.copy_(t)
        step()
        torch.cuda.synchronize()
        eager.append(loss_out.item())
    assert len(set(eager)) == 3 and all(math.isfinite(v) for v in eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    for t, want in zip(targets, eager):
        tgt.copy_(t)
        g.replay()
        torch.cuda.synchronize()
        assert abs(loss_out.item() - want) <= 2e-6 * max(1.0, abs(want)), (loss_out.item(), want)


def test_trainer_with_balanced_weights_and_unlabelled_training_nodes(tmp_path):
    """train_fixed_indices(loss=CrossEntropyLoss(weight=balanced, ignore_index=-1)) on the Cornell fixture of the reference
    loop, three epochs with the fixture's dropout masks, a fifth of the training nodes unlabelled: the loss trajectory is
    the oracle loop's (torch's loss with the same options, autograd, torch.optim.Adam) within the trajectory test's 1e-4."""
    import pathnet_amd
    from pathnet_amd import optim, trainer
    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refloop_hetero_cornell.npz")))
    Fg, H, C, W, L, E = int(g["F"]), int(g["H"]), int(g["C"]), int(g["W"]), int(g["L"]), 3
    p, lr, wd = float(g["p"]), float(g["lr"]), float(g["weight_decay"])
    X, Y = torch.as_tensor(g["X"]), torch.as_tensor(g["Y"]).clone()
    tr = np.flatnonzero(g["train_mask"])
    Y[torch.as_tensor(tr[::5])] = -1                        # unlabelled training nodes
    init = {k[5:]: torch.as_tensor(v) for k, v in g.items() if k.startswith("init.")}
    m = pathnet_amd.PathNet(Fg, H, C, L, dropout=p).cuda()
    m.load_state_dict(init)
    weight = optim.balanced_class_weight(Y[torch.as_tensor(tr)].cuda(), C, ignore_index=-1)
    fn = optim.CrossEntropyLoss(weight=weight, ignore_index=-1)
    losses = []
    plain = m.forward_loss

    def recording(*a, **kw):
        e = len(losses)
        m._mask_seq, m._mask_cls = torch.as_tensor(g["mask_seq%d" % e]).cuda(), torch.as_tensor(g["mask_cls%d" % e]).cuda()
        assert kw.get("loss") is fn
        loss, out = plain(*a, **kw)
        losses.append(loss.detach())
        return loss, out
    m.forward_loss = recording
    trainer.train_fixed_indices(X, Y, C, "cornell", g["train_mask"], g["val_mask"], g["test_mask"], W, H, L,
                                (torch.as_tensor(g["ids"][:E]), torch.as_tensor(g["codes"][:E])), epochs=E, lr=lr,
                                weight_decay=wd, dropout=p, device="cuda:0", save_dir=str(tmp_path), model=m, loss=fn)
    got = [v.item() for v in losses]
    pr = {k: v.clone().requires_grad_(True) for k, v in init.items()}
    opt = torch.optim.Adam(list(pr.values()), lr=lr, weight_decay=wd)
    want = []
    for e in range(E):
        out = po.forward("hetero", pr, X, g["ids"][e][tr], g["codes"][e][tr], tr, W, L,
                         drop_seq=torch.as_tensor(g["mask_seq%d" % e]), drop_cls=torch.as_tensor(g["mask_cls%d" % e]))
        lo = torch.nn.functional.cross_entropy(out, Y[torch.as_tensor(tr)], weight=weight.cpu(), ignore_index=-1)
        opt.zero_grad()
        lo.backward()
        opt.step()
        want.append(lo.item())
    print("trainer losses", got, "oracle", want)
    assert len(got) == E and max(abs(a - b) for a, b in zip(got, want)) < 1e-4, (got, want)
