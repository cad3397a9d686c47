"""The optimizer's options on the GPU -- pn_grad_norm, pn_adam_step_ex / pn_adam_step_ex_advance, pn_clip_grad_norm
(pn_optim.hip) and pathnet_amd.Adam / AdamW / LRSchedule / clip_grad_norm_ on top of them -- against the fp64 references
and derived bounds of tests/optim_options_ref.py, at the edges of the dispatch rules (tables there, held to the source by
tests/test_optim_options_host.py).

Norm: the fp64 sum of squares within (n + 64) 2^-53 of the reference.  Update: every element of every output within
adam_ex_ref's bound.  Every parameter, gradient and state array lives inside a sentinel-filled allocation (Guarded,
test_gpu_node_gemm.py) and must leave it as it was outside its own elements; the state buffer has sentinel words behind it."""
import copy
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import optim_options_ref as O
import optim_ref as R
from test_gpu_node_gemm import SENT, Guarded

pytestmark = pytest.mark.gpu
LR, (B1, B2), EPS, WD = O.HYPER
STATE_PAD = 8           # float64 sentinel words behind the state buffer
STATE_SENT = -7.25


def _lib():
    from pathnet_amd import _lib as L
    return L


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def device_state(adam_step, seed=0, epoch=0):
    """a pn_step_state in device memory"""
    return torch.tensor([epoch, seed, adam_step, 0], dtype=torch.int64, device="cuda")


class ExRun:
    """a list of (param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq) in guarded device allocations, a pn_optim state buffer,
    and the calls of the C ABI on them"""

    def __init__(self, host):
        L = _lib()
        self.host = [tuple(a.float().contiguous() for a in h) for h in host]
        self.dev = [tuple(Guarded((1, h[0].numel()), SENT, values=a) for a in h) for h in self.host]
        self.before = [[a.buf.clone() for a in d] for d in self.dev]
        n = len(self.dev)
        nbytes = ctypes.c_int64()
        L.check(L.load().pn_optim_state_bytes(sum(h[0].numel() for h in self.host), n, ctypes.byref(nbytes)))
        assert nbytes.value % 8 == 0
        self.words = nbytes.value // 8
        self.state = torch.zeros(self.words + STATE_PAD, dtype=torch.float64, device="cuda")
        self.state[self.words:] = STATE_SENT

    @classmethod
    def random(cls, counts, seed):
        return cls([O.warm_state(n, seed + 31 * i) for i, n in enumerate(counts)])

    def _plain(self):
        L = _lib()
        arr = (L.AdamTensor * max(len(self.dev), 1))()
        for i, (p, g, m, v, x) in enumerate(self.dev):
            arr[i] = L.AdamTensor(p.ptr(), g.ptr(), m.ptr(), v.ptr(), p.cols)
        return arr

    def norm(self):
        L = _lib()
        L.check(L.load().pn_grad_norm(self._plain(), len(self.dev), self.state.data_ptr(), _stream()))

    def clip(self, max_norm):
        L = _lib()
        L.check(L.load().pn_clip_grad_norm(self._plain(), len(self.dev), max_norm, self.state.data_ptr(), _stream()))

    def step(self, *, decoupled=False, amsgrad=False, max_norm=0.0, sched=None, step=1, step_state=None, advance=False,
             wd=WD):
        L = _lib()
        lib = L.load()
        flags = (L.OPTIM_DECOUPLED_WD if decoupled else 0) | (L.OPTIM_AMSGRAD if amsgrad else 0)
        spec = L.OptimSpec(flags=flags, max_grad_norm=max_norm, start_factor=1.0, step_size=1, gamma=1.0, t_max=1)
        if sched is not None:
            import pathnet_amd
            pathnet_amd.LRSchedule(**sched).fill(spec)
        n = len(self.dev)
        arr = (L.AdamTensorEx * max(n, 1))()
        for i, (p, g, m, v, x) in enumerate(self.dev):
            arr[i] = L.AdamTensorEx(p.ptr(), g.ptr(), m.ptr(), v.ptr(), x.ptr(), p.cols)
        sp = ctypes.c_void_p(step_state.data_ptr()) if step_state is not None else None
        if advance:
            L.check(lib.pn_adam_step_ex_advance(arr, n, LR, B1, B2, EPS, wd, ctypes.byref(spec), self.state.data_ptr(), sp,
                                                _stream()))
        else:
            L.check(lib.pn_adam_step_ex(arr, n, LR, B1, B2, EPS, wd, ctypes.byref(spec), self.state.data_ptr(), step, sp,
                                        _stream()))

    def report(self):
        """the pn_optim_report at the head of the state buffer, on the host; the words behind the buffer are untouched"""
        torch.cuda.synchronize()
        h = self.state.cpu()
        assert bool((h[self.words:] == STATE_SENT).all()), "wrote behind the state buffer"
        return {"norm": h[0].item(), "lr": h[1].item(), "coef": h[2:3].view(torch.float32)[0].item(),
                "coef_bits": h[2:3].view(torch.int32)[0].item(), "n_partials": h[2:3].view(torch.int32)[1].item(),
                "skipped": h[3:4].view(torch.int64)[0].item(), "norm_bits": h[0:1].view(torch.int64)[0].item()}

    def results(self, grads_untouched=True, amsgrad=True):
        """[(p, m, v, vmax)] on the host; nothing outside `count` moved, the gradients (and without amsgrad the running
        maximum) are bit for bit what they were"""
        torch.cuda.synchronize()
        out = []
        for i, d in enumerate(self.dev):
            hs = [a.host() for a in d]
            assert all(h.untouched_outside() for h in hs), "tensor %d: wrote past count" % i
            if grads_untouched:
                assert torch.equal(d[1].buf, self.before[i][1]), "tensor %d: the gradient was written" % i
            if not amsgrad:
                assert torch.equal(d[4].buf, self.before[i][4]), "tensor %d: max_exp_avg_sq written without amsgrad" % i
            out.append(tuple(hs[j].values()[0].clone() for j in (0, 2, 3, 4)))
        return out

    def unchanged(self):
        torch.cuda.synchronize()
        return all(torch.equal(a.buf, b) for d, bs in zip(self.dev, self.before) for a, b in zip(d, bs))

    def check(self, tag, step, *, decoupled=False, amsgrad=False, max_norm=None, lr_now=None, wd=WD):
        """the report's norm and coefficient within norm_ref / coef_ref's bounds (when a norm was asked for), every element
        of every output within adam_ex_ref's -> the report"""
        rep = self.report()
        coef, c_rel = 1.0, 0.0
        if max_norm is not None:
            norm, n_rel = O.norm_ref([h[1] for h in self.host])
            coef, c_rel = O.coef_ref(norm, max_norm, n_rel)
            print("%s: norm %.17g (ref %.17g, err/bound %.3g)  coef %.9g (ref %.9g)"
                  % (tag, rep["norm"], norm, abs(rep["norm"] - norm) / max(n_rel * norm, 1e-300), rep["coef"], coef))
            assert abs(rep["norm"] - norm) <= n_rel * norm, (tag, rep["norm"], norm)
            assert abs(rep["coef"] - coef) <= c_rel * coef, (tag, rep["coef"], coef)
        else:
            assert math.isnan(rep["norm"]) and rep["coef"] == 1.0
        assert rep["skipped"] == 0
        worst = 0.0
        for i, (h, got) in enumerate(zip(self.host, self.results(amsgrad=amsgrad))):
            ref, bounds = O.adam_ex_ref(h[0], h[1], h[2], h[3], h[4], step, LR, B1, B2, EPS, wd, decoupled=decoupled,
                                        amsgrad=amsgrad, coef=coef, coef_rel=c_rel, lr_now=lr_now)
            for name, a, r, b in zip(("p", "m", "v", "vmax"), got, ref, bounds):
                if r is None:
                    continue
                assert torch.isfinite(a).all(), (tag, i, name)
                err = (a.double() - r).abs()
                if err.numel():
                    worst = max(worst, (err / b.clamp_min(1e-300)).max().item())
                assert bool((err <= b).all()), "%s: tensor %d %s' off by %.3g of its bound" % (
                    tag, i, name, (err / b.clamp_min(1e-300)).max().item())
        print("%s: worst err / bound = %.3g" % (tag, worst))
        return rep


def _norm_then_step(run, tag, step=3, factor=0.5):
    """pn_grad_norm, then a clipped amsgrad update at max_norm = factor * the reference norm; everything within bound"""
    norm = O.norm_ref([h[1] for h in run.host])[0]
    max_norm = R.f32(factor * norm) if norm > 0 else 1.0
    run.norm()
    run.step(amsgrad=True, max_norm=max_norm, step=step)
    return run.check(tag, step, amsgrad=True, max_norm=max_norm)


# ------------------------------------------------------------------------------------------------
# the norm at its edges
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", O.NORM_COUNTS)
def test_norm_element_count_edges(count):
    rep = _norm_then_step(ExRun.random([count], seed=count), "count %d" % count)
    assert rep["n_partials"] == min(-(-count // O.OPT_CHUNK), O.OPT_GRID_CAP) and rep["coef"] < 1.0


@pytest.mark.parametrize("n", O.NORM_LIST_LENGTHS)
def test_norm_tensor_count_edges(n):
    rep = _norm_then_step(ExRun.random([17] * n, seed=n), "%d tensors" % n)
    assert rep["n_partials"] == n           # one chunk per tensor: the partials of the later launches lie behind the first 32


@pytest.mark.parametrize("counts", O.NORM_ZERO_POSITIONS)
def test_norm_zero_element_tensor_in_a_list(counts):
    _norm_then_step(ExRun.random(list(counts), seed=sum(c * (i + 1) for i, c in enumerate(counts))), "counts %r" % (counts,))


def test_norm_of_an_empty_list_and_of_empty_tensors():
    for counts in ([], [0], [0] * 33):
        run = ExRun.random(counts, seed=1)
        run.norm()
        run.step(max_norm=1.0, step=1)
        rep = run.report()
        assert rep["norm"] == 0.0 and rep["coef"] == 1.0 and rep["n_partials"] == 1 and rep["skipped"] == 0, (counts, rep)
        assert run.unchanged()


def test_norm_all_zero_gradients():
    p, g, m, v, x = O.warm_state(300, 2)
    run = ExRun([(p, torch.zeros_like(g), m, v, x)])
    run.norm()
    run.step(max_norm=1.0, step=2)
    rep = run.check("zero gradients", 2, max_norm=1.0)
    assert rep["norm"] == 0.0 and rep["coef"] == 1.0


def test_norm_where_the_fp32_square_overflows():
    """elements of 1e25: 1e50 is no float, the fp64 sum is fine -- a finite norm, the coefficient of the reference, and an
    update on the clipped gradient within bound"""
    p, g, m, v, x = O.warm_state(300, 3)
    big = torch.full_like(g, 1e25) * torch.where(torch.arange(300) % 2 == 0, 1.0, -1.0)
    assert torch.isinf(big * big).all()
    run = ExRun([(p, big, m, v, x)])
    run.norm()
    run.step(max_norm=1.0, step=2)
    rep = run.check("1e25", 2, max_norm=1.0)
    assert math.isfinite(rep["norm"]) and abs(rep["norm"] - math.sqrt(300.0) * R.f32(1e25)) <= 1e-12 * rep["norm"]
    assert 0.0 < rep["coef"] < 1e-25


def test_same_inputs_twice_give_the_same_bits():
    counts = [17] * 33 + [5000, 0, 2049]
    reps, outs = [], []
    for _ in range(2):
        run = ExRun.random(counts, seed=12)
        rep = _norm_then_step(run, "determinism")
        reps.append((rep["norm_bits"], rep["coef_bits"], rep["n_partials"]))
        outs.append(run.results())
    assert reps[0] == reps[1]
    for a, b in zip(outs[0], outs[1]):
        for s, t in zip(a, b):
            assert torch.equal(s, t)


# ------------------------------------------------------------------------------------------------
# the update
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoupled,amsgrad,clip", O.UPDATE_COMBOS)
def test_update_combinations_from_an_arbitrary_state(decoupled, amsgrad, clip):
    """{L2, decoupled} x {amsgrad off, on} x {no clip, clip active, clip inactive} on the element classes of
    optim_ref.adam_elements(), the step count given by the host and read from a device pn_step_state"""
    host = O.elements_state()
    norm = O.norm_ref([host[1]])[0]
    mode = O.CLIP_MODES[clip]
    max_norm = None if mode is None else R.f32(mode * norm)
    for step in (1, 10):
        for state in (None, device_state(step, seed=5, epoch=9)):
            run = ExRun([host])
            if max_norm is not None:
                run.norm()
            run.step(decoupled=decoupled, amsgrad=amsgrad, max_norm=max_norm or 0.0, step=step if state is None else 1,
                     step_state=state)
            tag = "%s %s clip=%s step %d (%s count)" % ("decoupled" if decoupled else "L2", "amsgrad" if amsgrad else "plain",
                                                        clip, step, "host" if state is None else "device")
            rep = run.check(tag, step, decoupled=decoupled, amsgrad=amsgrad, max_norm=max_norm)
            assert rep["lr"] == R.f32(LR)
            if clip != "none":
                assert (rep["coef"] < 1.0) == (clip == "active")
            if state is not None:
                assert state.tolist() == [9, 5, step, 0]        # pn_adam_step_ex moves nothing


def test_every_option_off_agrees_with_pn_adam_step():
    """flags 0, no clip, constant schedule: torch.optim.Adam's update like pn_adam_step's -- both inside adam_ref's bound, so
    within twice the bound of each other (the bias corrections are formed by squaring here and by pow there, and the
    compiler may contract other products: not the same bits)"""
    L = _lib()
    host = [O.warm_state(n, n) for n in (300, 2049, 17)]
    ex = ExRun(host)
    ex.step(step=4)
    ex.check("options off", 4)
    plain = ExRun(host)
    L.check(L.load().pn_adam_step(plain._plain(), 3, LR, B1, B2, EPS, WD, 4, None, _stream()))
    for h, a, b in zip(host, ex.results(amsgrad=False), plain.results(amsgrad=False)):
        bounds = R.adam_ref(h[0], h[1], h[2], h[3], 4, LR, B1, B2, EPS, WD)[1]
        for s, t, e in zip(a, b, bounds):
            assert bool(((s.double() - t.double()).abs() <= 2 * e).all())


def test_advance_twin_moves_the_state_once():
    """33 tensors, the 33rd spanning three workgroups, then 32 + an empty 33rd, through pn_adam_step_ex_advance: the update
    used the count before the advance, one advance, the ticket word back at zero"""
    for last in (4097, 0):
        run = ExRun.random([17] * 32 + [last], seed=34)
        state = device_state(3, seed=123, epoch=0)
        run.norm()
        run.step(amsgrad=True, max_norm=1.0, step_state=state, advance=True)
        run.check("advance, last of %d" % last, 3, amsgrad=True, max_norm=1.0)
        e, s, a, r = state.tolist()
        assert {"epoch": e, "seed": s & R.MASK64, "adam_step": a} == R.splitmix_advance({"epoch": 0, "seed": 123, "adam_step": 3})
        assert r == 0


def test_argument_errors():
    L = _lib()
    lib = L.load()
    run = ExRun.random([17], seed=1)
    t = L.AdamTensorEx(run.dev[0][0].ptr(), run.dev[0][1].ptr(), run.dev[0][2].ptr(), run.dev[0][3].ptr(), None, 17)
    arr = (L.AdamTensorEx * 1)(t)
    ok = dict(flags=0, max_grad_norm=0.0, start_factor=1.0, step_size=1, gamma=1.0, t_max=1)
    bad = [dict(ok, flags=8), dict(ok, max_grad_norm=-1.0), dict(ok, max_grad_norm=float("nan")), dict(ok, schedule=4),
           dict(ok, warmup_steps=-1), dict(ok, start_factor=1.5), dict(ok, schedule=L.LR_STEP, step_size=0),
           dict(ok, schedule=L.LR_EXPONENTIAL, gamma=0.0), dict(ok, schedule=L.LR_COSINE, t_max=0),
           dict(ok, schedule=L.LR_COSINE, lr_min=1.0), dict(ok, flags=L.OPTIM_AMSGRAD)]      # (the last: no max_exp_avg_sq)
    for kw in bad:
        rc = lib.pn_adam_step_ex(arr, 1, LR, B1, B2, EPS, WD, ctypes.byref(L.OptimSpec(**kw)), run.state.data_ptr(), 1, None,
                                 _stream())
        assert rc == L.PN_ERR_ARG and lib.pn_last_error(), kw
    spec = L.OptimSpec(**dict(ok, max_grad_norm=1.0))
    assert lib.pn_adam_step_ex(arr, 1, LR, B1, B2, EPS, WD, ctypes.byref(spec), None, 1, None, _stream()) == L.PN_ERR_ARG
    assert lib.pn_adam_step_ex(arr, 1, LR, B1, B2, EPS, WD, None, run.state.data_ptr(), 1, None, _stream()) == L.PN_ERR_ARG
    assert lib.pn_adam_step_ex(arr, 1, LR, B1, B2, EPS, WD, ctypes.byref(L.OptimSpec(**ok)), None, 0, None, _stream()) == L.PN_ERR_ARG
    assert lib.pn_adam_step_ex_advance(arr, 1, LR, B1, B2, EPS, WD, ctypes.byref(L.OptimSpec(**ok)), None, None,
                                       _stream()) == L.PN_ERR_ARG
    assert lib.pn_grad_norm(run._plain(), 1, None, _stream()) == L.PN_ERR_ARG
    assert lib.pn_clip_grad_norm(run._plain(), 1, 0.0, run.state.data_ptr(), _stream()) == L.PN_ERR_ARG
    assert lib.pn_optim_state_bytes(-1, 1, ctypes.byref(ctypes.c_int64())) == L.PN_ERR_ARG
    assert run.unchanged()


# ------------------------------------------------------------------------------------------------
# gradients: untouched by the fused clip, scaled by the stand-alone one
# ------------------------------------------------------------------------------------------------
def _params(shapes, seed):
    gen = torch.Generator().manual_seed(seed)
    init = [torch.randn(*s, generator=gen) for s in shapes]
    return init, [torch.nn.Parameter(p.clone().cuda()) for p in init]


def test_fused_clip_leaves_the_gradients_and_clip_grad_norm_scales_them():
    import pathnet_amd
    shapes = [(300,), (5, 7), (1,), (2049,)] + [(17,)] * 30
    init, ps = _params(shapes, 21)
    gen = torch.Generator().manual_seed(22)
    grads = [torch.randn(*s, generator=gen) for s in shapes]
    for p, g in zip(ps, grads):
        p.grad = g.clone().cuda()
    norm, n_rel = O.norm_ref(grads)
    opt = pathnet_amd.Adam(ps, lr=LR, weight_decay=WD, max_grad_norm=1.0)
    opt.step()
    torch.cuda.synchronize()
    for p, g in zip(ps, grads):
        assert torch.equal(p.grad.cpu(), g)             # bit for bit
    assert abs(opt.last_grad_norm.item() - norm) <= n_rel * norm and opt.last_grad_norm.dtype == torch.float64
    coef, c_rel = O.coef_ref(norm, 1.0, n_rel)
    assert coef < 1.0 and abs(opt.last_clip_coef.item() - coef) <= c_rel * coef
    assert opt.skipped_steps.item() == 0 and opt.last_lr.item() == R.f32(LR)
    # the stand-alone clip: in place, coef * g within one rounding of the product and the coefficient's own bound
    total = pathnet_amd.clip_grad_norm_(ps, 1.0)
    assert total.is_cuda and total.dim() == 0
    assert abs(total.item() - norm) <= n_rel * norm
    for p, g in zip(ps, grads):
        want = coef * g.double()
        assert bool(((p.grad.cpu().double() - want).abs() <= (R.U + c_rel) * want.abs()).all())
    # already inside the ball: nothing moves
    clipped = [p.grad.clone() for p in ps]
    total2 = pathnet_amd.clip_grad_norm_(ps, 10.0)
    assert abs(total2.item() - 1.0) <= 1e-5
    for p, c in zip(ps, clipped):
        assert torch.equal(p.grad, c)
    # a single tensor, and a list without gradients
    one = pathnet_amd.clip_grad_norm_(ps[0], 1e-3)
    assert abs(ps[0].grad.norm().item() - 1e-3) <= 1e-8 and one.item() > 1e-3
    assert pathnet_amd.clip_grad_norm_([torch.nn.Parameter(torch.zeros(3).cuda())], 1.0).item() == 0.0


@pytest.mark.parametrize("counts", ([17] * 33 + [4097], [0, 2049, 0]))
def test_clip_grad_norm_through_the_c_abi(counts):
    """pn_clip_grad_norm on guarded lists: coef * g within bound, nothing but the gradients' own elements written"""
    run = ExRun.random(counts, seed=61)
    norm, n_rel = O.norm_ref([h[1] for h in run.host])
    max_norm = R.f32(0.25 * norm)
    coef, c_rel = O.coef_ref(norm, max_norm, n_rel)
    run.clip(max_norm)
    rep = run.report()
    assert abs(rep["norm"] - norm) <= n_rel * norm and abs(rep["coef"] - coef) <= c_rel * coef and rep["skipped"] == 0
    for d, bs, h in zip(run.dev, run.before, run.host):
        for j in (0, 2, 3, 4):
            assert torch.equal(d[j].buf, bs[j])
        gh = d[1].host()
        want = coef * h[1].double()
        assert gh.untouched_outside() and bool(((gh.values()[0].double() - want).abs() <= (R.U + c_rel) * want.abs()).all())


# ------------------------------------------------------------------------------------------------
# the non-finite guard
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad,mode", (("inf", "clip"), ("nan", "clip"), ("inf", "guard"), ("nan", "guard")))
def test_non_finite_gradient_skips_the_step(bad, mode):
    """one inf / NaN in one gradient of a 33-tensor list: every p, m, v, vmax keeps its bits and skipped_steps == 1; the
    finite step that follows updates at ITS step count (3: the skipped step used up the 2)"""
    import pathnet_amd
    shapes = [(17,)] * 33
    init, ps = _params(shapes, 41)
    gen = torch.Generator().manual_seed(42)
    grads = [[torch.randn(*s, generator=gen) for s in shapes] for _ in range(3)]
    grads[1][20][3] = float(bad)
    max_norm = 1.0 if mode == "clip" else None
    opt = pathnet_amd.AdamW(ps, lr=LR, weight_decay=WD, amsgrad=True, max_grad_norm=max_norm, skip_nonfinite=mode == "guard")
    cur = [(p.double(), torch.zeros_like(p).double(), torch.zeros_like(p).double(), torch.zeros_like(p).double()) for p in init]
    errs = [None] * len(init)
    for k in range(3):
        for p, g in zip(ps, grads[k]):
            p.grad = g.clone().cuda()
        if k == 1:
            before = [(p.detach().clone(),) + tuple(opt.state[p][key].clone() for key in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"))
                      for p in ps]
        opt.step()
        torch.cuda.synchronize()
        if k == 1:
            assert opt.skipped_steps.item() == 1 and not math.isfinite(opt.last_grad_norm.item())
            assert opt.last_clip_coef.item() == 1.0
            for p, b in zip(ps, before):
                st = opt.state[p]
                for a, c in zip((p.detach(), st["exp_avg"], st["exp_avg_sq"], st["max_exp_avg_sq"]), b):
                    assert torch.equal(a.view(torch.int32), c.view(torch.int32))
            continue
        norm, n_rel = O.norm_ref(grads[k])
        coef, c_rel = O.coef_ref(norm, max_norm, n_rel)
        assert (coef < 1.0) == (mode == "clip")
        for i in range(len(init)):
            cur[i], errs[i] = O.adam_ex_ref(cur[i][0], grads[k][i], cur[i][1], cur[i][2], cur[i][3], k + 1, LR, B1, B2, EPS, WD,
                                            decoupled=True, amsgrad=True, coef=coef, coef_rel=c_rel, err=errs[i])
    assert opt.skipped_steps.item() == 1 and all(opt.state[p]["step"] == 3 for p in ps)
    for i, p in enumerate(ps):
        st = opt.state[p]
        for a, r, b in zip((p.detach(), st["exp_avg"], st["exp_avg_sq"], st["max_exp_avg_sq"]), cur[i], errs[i]):
            assert bool(((a.cpu().double() - r).abs() <= b).all()), i


# ------------------------------------------------------------------------------------------------
# the schedule
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(O.SCHEDULES))
def test_schedule_on_the_device(name):
    """last_lr at the schedule's corners and at step 10^6, the count given by the host and read from a StepState, within
    1e-12 relative of lr_ref; the parameters follow adam_ex_ref at that rate"""
    import pathnet_amd
    sched = O.SCHEDULES[name]
    host = O.warm_state(33, 7)
    for step in O.SCHEDULE_STEPS:
        want = O.lr_ref(LR, step, **sched)
        run = ExRun([host])
        run.step(sched=sched, step=step)
        rep = run.check("%s step %d" % (name, step), step, lr_now=want)
        assert abs(rep["lr"] - want) <= 1e-12 * want, (name, step, rep["lr"], want)
        # pathnet_amd.Adam with a StepState: the same value from the device count
        st = pathnet_amd.StepState("cuda", seed=1)
        st.t[2] = step
        p = torch.nn.Parameter(host[0].clone().cuda())
        p.grad = host[1].clone().cuda()
        opt = pathnet_amd.Adam([p], lr=LR, weight_decay=WD, step_state=st, schedule=pathnet_amd.LRSchedule(**sched))
        opt.step()
        got = opt.last_lr.item()
        assert abs(got - want) <= 1e-12 * want and got == rep["lr"], (name, step, got, want)
        assert abs(pathnet_amd.LRSchedule(**sched).lr_at(LR, step) - want) <= 1e-15 * want


# ------------------------------------------------------------------------------------------------
# the captured step
# ------------------------------------------------------------------------------------------------
def test_captured_step_with_clip_schedule_and_amsgrad_follows_the_reference():
    """`st.advance(); opt.step()` with clipping, a warm-up + cosine schedule and amsgrad, captured after a warm-up step and
    replayed six times with refilled gradients, one of them holding an inf: the parameters and the state equal
    adam_ex_ref iterated at steps 2 .. 7 with the same skip, within the bounds added up along the trajectory, and last_lr
    moves from replay to replay -- a learning rate baked into the capture fails here."""
    import pathnet_amd
    sched = dict(kind="cosine", warmup_steps=2, start_factor=0.25, t_max=10, lr_min=1e-4)
    shapes = [(300,), (5, 7), (1,)]
    init, ps = _params(shapes, 8)
    gen = torch.Generator().manual_seed(9)
    grads = [[torch.randn(*s, generator=gen) for s in shapes] for _ in range(7)]
    grads[4][1][2, 3] = float("inf")
    static = [g.clone().cuda() for g in grads[0]]
    for p, g in zip(ps, static):
        p.grad = g
    st = pathnet_amd.StepState("cuda", seed=2)
    opt = pathnet_amd.Adam(ps, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD, step_state=st, amsgrad=True, max_grad_norm=1.0,
                           schedule=pathnet_amd.LRSchedule(**sched))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):           # warm-up = step 1 (creates the optimizer state and its device buffer)
        st.advance()
        opt.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    lrs = [opt.last_lr.item()]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st.advance()
        opt.step()
    assert st.values()["adam_step"] == 1
    skipped = []
    for k in range(1, 7):
        for s, g in zip(static, grads[k]):
            s.copy_(g)
        graph.replay()
        torch.cuda.synchronize()
        lrs.append(opt.last_lr.item())
        skipped.append(opt.skipped_steps.item())
    assert st.values()["adam_step"] == 7 and skipped == [0, 0, 0, 1, 1, 1]
    want_lrs = [O.lr_ref(LR, k + 1, **sched) for k in range(7)]
    assert len(set(lrs)) == 7
    for got, want in zip(lrs, want_lrs):
        assert abs(got - want) <= 1e-12 * want, (lrs, want_lrs)
    worst = 0.0
    coefs = []
    for k in range(7):
        norm, n_rel = O.norm_ref(grads[k])
        coefs.append(O.coef_ref(norm, 1.0, n_rel) if math.isfinite(norm) else None)
    assert coefs[4] is None and all(c[0] < 1.0 for c in coefs if c is not None)
    for i, p0 in enumerate(init):
        z = torch.zeros_like(p0).double()
        cur, err = (p0.double(), z, z, z), None
        for k in range(7):
            if coefs[k] is None:
                continue                    # the skipped step: values and bounds carry over
            cur, err = O.adam_ex_ref(cur[0], grads[k][i], cur[1], cur[2], cur[3], k + 1, LR, B1, B2, EPS, WD, amsgrad=True,
                                     coef=coefs[k][0], coef_rel=coefs[k][1], lr_now=want_lrs[k], err=err)
        stt = opt.state[ps[i]]
        for a, r, b in zip((ps[i].detach(), stt["exp_avg"], stt["exp_avg_sq"], stt["max_exp_avg_sq"]), cur, err):
            e = (a.cpu().double() - r).abs()
            worst = max(worst, (e / b.clamp_min(1e-300)).max().item())
            assert bool((e <= b).all()), (i, (e / b.clamp_min(1e-300)).max().item())
    print("six replays: worst err / summed bound = %.3g" % worst)


# ------------------------------------------------------------------------------------------------
# the default route
# ------------------------------------------------------------------------------------------------
def test_an_optimizer_without_options_takes_the_old_calls(monkeypatch):
    """pathnet_amd.Adam() with no option set issues pn_adam_step / pn_adam_step_advance and nothing else of the optimizer's
    symbols; its result has the bits of a direct pn_adam_step on the same values and lies within optim_ref.adam_ref's bound"""
    import pathnet_amd
    L = _lib()
    lib = L.load()
    calls = []
    names = [n for n in L.SIGNATURES if n.startswith(("pn_adam", "pn_grad_norm", "pn_clip", "pn_optim"))]
    assert len(names) == 7

    def counted(name, fn):
        def call(*a):
            calls.append(name)
            return fn(*a)
        return call
    for n in names:
        monkeypatch.setattr(lib, n, counted(n, getattr(lib, n)))
    host = [O.warm_state(n, n)[:2] for n in (300, 2049, 17)]
    ps = [torch.nn.Parameter(h[0].clone().cuda()) for h in host]
    for p, h in zip(ps, host):
        p.grad = h[1].clone().cuda()
    opt = pathnet_amd.Adam(ps, lr=LR, weight_decay=WD)
    opt.step()
    st = pathnet_amd.StepState("cuda", seed=3, advance_in_adam=True)
    qs = [torch.nn.Parameter(h[0].clone().cuda()) for h in host]
    for q, h in zip(qs, host):
        q.grad = h[1].clone().cuda()
    st.advance()
    opt2 = pathnet_amd.Adam(qs, lr=LR, weight_decay=WD, step_state=st)
    opt2.step()
    torch.cuda.synchronize()
    assert calls == ["pn_adam_step", "pn_adam_step_advance"] and opt._optim_state is None and opt.last_lr is None
    monkeypatch.undo()
    direct = ExRun([(h[0], h[1], torch.zeros_like(h[0]), torch.zeros_like(h[0]), torch.zeros_like(h[0])) for h in host])
    L.check(lib.pn_adam_step(direct._plain(), 3, LR, B1, B2, EPS, WD, 1, None, _stream()))
    for p, q, h, d in zip(ps, qs, host, direct.results(amsgrad=False)):
        assert torch.equal(p.detach().cpu(), d[0]) and torch.equal(q.detach().cpu(), d[0])
        assert torch.equal(opt.state[p]["exp_avg"].cpu(), d[1]) and torch.equal(opt.state[p]["exp_avg_sq"].cpu(), d[2])
        z = torch.zeros_like(h[0])
        ref, bound = R.adam_ref(h[0], h[1], z, z, 1, LR, B1, B2, EPS, WD)
        assert bool(((d[0].double() - ref[0]).abs() <= bound[0]).all())
        assert set(opt.state[p]) == {"step", "exp_avg", "exp_avg_sq"}


# ------------------------------------------------------------------------------------------------
# state_dict with torch, on the device
# ------------------------------------------------------------------------------------------------
def test_state_of_torch_adamw_amsgrad_continues_here():
    """three steps of torch.optim.AdamW(amsgrad=True) on the GPU, its state_dict loaded into pathnet_amd.AdamW, a fourth
    step on both: the same parameters within the fourth step's bound"""
    import pathnet_amd
    init, ps = _params([(300,), (5, 7)], 51)
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    gen = torch.Generator().manual_seed(52)
    topt = torch.optim.AdamW(ps, lr=LR, weight_decay=1e-2, amsgrad=True)
    for k in range(4):
        gs = [torch.randn(*p.shape, generator=gen) for p in ps]
        if k == 3:
            ours = pathnet_amd.AdamW(qs, lr=LR, amsgrad=True)
            ours.load_state_dict(copy.deepcopy(topt.state_dict()))
            for q, p in zip(qs, ps):
                q.data.copy_(p.data)
            start = [(p.detach().cpu(),) + tuple(topt.state[p][key].cpu() for key in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"))
                     for p in ps]
            for q, g in zip(qs, gs):
                q.grad = g.cuda()
            ours.step()
        for p, g in zip(ps, gs):
            p.grad = g.cuda()
        topt.step()
    torch.cuda.synchronize()
    for q, s, g in zip(qs, start, gs):
        assert ours.state[q]["step"] == 4 and set(ours.state[q]) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}
        ref, bound = O.adam_ex_ref(s[0], g, s[1], s[2], s[3], 4, LR, B1, B2, EPS, 1e-2, decoupled=True, amsgrad=True)
        assert bool(((q.detach().cpu().double() - ref[0]).abs() <= bound[0]).all())


# ------------------------------------------------------------------------------------------------
# the trainer
# ------------------------------------------------------------------------------------------------
def test_trainer_takes_an_optimizer_factory(tmp_path):
    """train_fixed_indices(optimizer=...) on the Cornell fixture for three epochs with AdamW, clipping and a warm-up + cosine
    schedule: the factory is called once with the model's parameters, last_lr ends at the schedule's third step, and the
    five metrics are finite"""
    import pathnet_amd
    from pathnet_amd import trainer
    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refloop_hetero_cornell.npz")))
    Fg, H, C, W, L, E = int(g["F"]), int(g["H"]), int(g["C"]), int(g["W"]), int(g["L"]), 3
    m = pathnet_amd.PathNet(Fg, H, C, L, dropout=float(g["p"])).cuda()
    sched = dict(kind="cosine", warmup_steps=1, t_max=3)
    made = []

    def factory(params):
        params = list(params)
        made.append((params, pathnet_amd.AdamW(params, lr=0.005, max_grad_norm=1.0, schedule=pathnet_amd.LRSchedule(**sched))))
        return made[-1][1]
    res = trainer.train_fixed_indices(torch.as_tensor(g["X"]), torch.as_tensor(g["Y"]), C, "cornell", g["train_mask"],
                                      g["val_mask"], g["test_mask"], W, H, L,
                                      (torch.as_tensor(g["ids"][:E]), torch.as_tensor(g["codes"][:E])), epochs=E,
                                      device="cuda:0", save_dir=str(tmp_path), model=m, optimizer=factory)
    assert len(made) == 1
    params, opt = made[0]
    assert len(params) == len(list(m.parameters())) and all(a is b for a, b in zip(params, m.parameters()))
    want = O.lr_ref(0.005, 3, **sched)
    assert abs(opt.last_lr.item() - want) <= 1e-12 * want
    assert opt.skipped_steps.item() == 0 and math.isfinite(opt.last_grad_norm.item()) and 0.0 < opt.last_clip_coef.item() <= 1.0
    assert len(res) == 5 and all(math.isfinite(r) for r in res)
