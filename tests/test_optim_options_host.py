"""The optimizer's options on the CPU (no GPU): the fp64 references of tests/optim_options_ref.py against torch's own
float64 implementations, the derived bounds against a faithful fp32 evaluation of the kernel's operation order, the
constructors' validation, and the case tables of tests/test_gpu_optim_options.py against the dispatch constants of
pn_optim.hip."""
import math
import os
import re

import pytest
import torch

import optim_options_ref as O
import optim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, (B1, B2), EPS, WD = O.HYPER


def _rel(a, b):
    return ((a - b).abs() / b.abs().clamp_min(1e-300)).max().item()


@pytest.mark.parametrize("amsgrad", (False, True))
@pytest.mark.parametrize("decoupled", (False, True))
def test_adam_ex_ref_equals_torch_in_float64(decoupled, amsgrad):
    """20 steps of random gradients against torch.optim.AdamW / torch.optim.Adam(amsgrad=True) in float64, constructed with
    the same float32-rounded hyper-parameters: 1e-12 relative"""
    torch.manual_seed(4)
    shapes = [(37, 5), (1,), (300,)]
    ref = [torch.nn.Parameter(torch.randn(*s, dtype=torch.float64)) for s in shapes]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    wd = 1e-2 if decoupled else WD
    opt = cls(ref, lr=R.f32(LR), betas=(R.f32(B1), R.f32(B2)), eps=R.f32(EPS), weight_decay=R.f32(wd), amsgrad=amsgrad,
              foreach=False)
    ours = [(q.detach().clone(), torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(q)) for q in ref]
    for step in range(1, 21):
        for i, q in enumerate(ref):
            g = torch.randn(*q.shape, dtype=torch.float64)
            q.grad = g.clone()
            p, m, v, x = ours[i]
            ours[i] = O.adam_ex_ref(p, g, m, v, x, step, LR, B1, B2, EPS, wd, decoupled=decoupled, amsgrad=amsgrad)[0]
        opt.step()
    for q, (p, m, v, x) in zip(ref, ours):
        st = opt.state[q]
        assert _rel(p, q.detach()) <= 1e-12 and _rel(m, st["exp_avg"]) <= 1e-12 and _rel(v, st["exp_avg_sq"]) <= 1e-12
        if amsgrad:
            assert _rel(x, st["max_exp_avg_sq"]) <= 1e-12
        else:
            assert x is None


def test_adam_ex_ref_without_options_is_adam_ref():
    p, g, m, v = R.adam_elements()
    want, wb = R.adam_ref(p, g, m, v, 7, LR, B1, B2, EPS, WD)
    got, gb = O.adam_ex_ref(p, g, m, v, None, 7, LR, B1, B2, EPS, WD)
    for a, b in zip(want + wb, got[:3] + gb[:3]):
        assert torch.equal(a, b)


def test_norm_and_coef_ref_equal_clip_grad_norm_in_float64():
    torch.manual_seed(5)
    for scale, max_norm in ((1.0, 1.0), (1e-3, 1.0), (100.0, 0.5), (1.0, 1e6)):
        ps = [torch.nn.Parameter(torch.zeros(s, dtype=torch.float64)) for s in ((33, 3), (1,), (257,))]
        for q in ps:
            # float32 values in float64 tensors: what the kernel sees, and norm_ref's squares stay exact
            q.grad = (scale * torch.randn(*q.shape)).float().double()
        before = [q.grad.clone() for q in ps]
        total = torch.nn.utils.clip_grad_norm_(ps, R.f32(max_norm), foreach=False).item()
        norm, rel = O.norm_ref(before)
        assert abs(norm - total) <= 1e-12 * total and 0 < rel < 1e-12
        coef, c_rel = O.coef_ref(norm, max_norm, rel)
        assert 0 < c_rel < 2 * R.U
        for q, b in zip(ps, before):
            assert _rel(coef * b, q.grad) <= 1e-12
    assert O.coef_ref(3.0, None) == (1.0, 0.0) and O.coef_ref(3.0, math.inf) == (1.0, 0.0)
    assert O.norm_ref([torch.zeros(5)])[0] == 0.0 and O.coef_ref(0.0, 1.0)[0] == 1.0
    big = O.norm_ref([torch.full((4,), 1e25)])[0]
    assert math.isfinite(big) and abs(big - 2e25) <= 1e-6 * 2e25         # (1e25 is not a float: its neighbour's norm)


def _torch_schedule(name, steps):
    """[lr of step 1 .. steps] from torch's own schedulers at the fp32-rounded base rate (float64 arithmetic: Python floats)"""
    s = O.SCHEDULES[name]
    q = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([q], lr=R.f32(LR))
    sched = torch.optim.lr_scheduler
    warm = sched.LinearLR(opt, start_factor=s["start_factor"], end_factor=1.0, total_iters=s["warmup_steps"])
    if name == "constant":
        main = sched.ConstantLR(opt, factor=1.0, total_iters=0)
    elif name == "step":
        main = sched.StepLR(opt, step_size=s["step_size"], gamma=s["gamma"])
    elif name == "exponential":
        main = sched.ExponentialLR(opt, gamma=s["gamma"])
    else:
        main = sched.CosineAnnealingLR(opt, T_max=s["t_max"], eta_min=s["lr_min"])
    both = sched.SequentialLR(opt, [warm, main], milestones=[s["warmup_steps"]])
    out = []
    for _ in range(steps):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        both.step()
    return out


@pytest.mark.parametrize("name", sorted(O.SCHEDULES))
def test_lr_ref_equals_torch_schedulers(name):
    """LinearLR warm-up, then StepLR / ExponentialLR / CosineAnnealingLR (up to t_max), chained by SequentialLR"""
    s = O.SCHEDULES[name]
    steps = s["warmup_steps"] + O.T_MAX + 1         # e - warmup <= t_max
    want = _torch_schedule(name, steps)
    for k, w in enumerate(want, start=1):
        got = O.lr_ref(LR, k, **s)
        assert abs(got - w) <= 1e-12 * abs(w), (name, k, got, w)


def test_lr_ref_cosine_closed_form_and_clamp():
    s = dict(kind="cosine", t_max=O.T_MAX, lr_min=1e-4)
    q = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([q], lr=R.f32(LR))
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=O.T_MAX, eta_min=1e-4)
    for e in range(O.T_MAX + 1):
        sched.last_epoch = e
        want = sched._get_closed_form_lr()[0]
        assert abs(O.lr_ref(LR, e + 1, **s) - want) <= 1e-12 * want
    # after t_max: held at lr_min (torch's recursion turns upwards again there)
    assert O.lr_ref(LR, O.T_MAX + 1, **s) == O.lr_ref(LR, O.T_MAX + 2, **s) == O.lr_ref(LR, 10 ** 6, **s)
    assert abs(O.lr_ref(LR, 10 ** 6, **s) - 1e-4) <= 1e-16


@pytest.mark.parametrize("name", sorted(O.SCHEDULES))
def test_lr_schedule_lr_at_equals_lr_ref(name):
    import pathnet_amd
    s = O.SCHEDULES[name]
    sch = pathnet_amd.LRSchedule(**s)
    for step in O.SCHEDULE_STEPS + tuple(range(1, 60)):
        want = O.lr_ref(LR, step, **s)
        assert abs(sch.lr_at(LR, step) - want) <= 1e-15 * want, (name, step)
    assert pathnet_amd.LRSchedule().lr_at(LR, 9) == R.f32(LR)


@pytest.mark.parametrize("decoupled,amsgrad,clip", O.UPDATE_COMBOS)
def test_fp32_evaluation_stays_inside_the_bound(decoupled, amsgrad, clip):
    """the kernel's operation order in fp32 on the CPU against adam_ex_ref: the bound is achievable, on the element table
    of the GPU test and on random warm states, at an early and a late step and under a schedule"""
    tables = [("elements", O.elements_state())] + [("random%d" % n, O.warm_state(n, n)) for n in (257, 2049)]
    for tag, (p, g, m, v, x) in tables:
        norm, n_rel = O.norm_ref([g])
        mode = O.CLIP_MODES[clip]
        coef, c_rel = O.coef_ref(norm, None if mode is None else mode * norm, n_rel)
        assert (coef < 1.0) == (clip == "active")
        for step, lr_now in ((1, None), (3, O.lr_ref(LR, 3, **O.SCHEDULES["cosine"])), (1000, None)):
            kw = dict(decoupled=decoupled, amsgrad=amsgrad, coef=coef, lr_now=lr_now)
            ref, bound = O.adam_ex_ref(p, g, m, v, x, step, LR, B1, B2, EPS, WD, coef_rel=c_rel, **kw)
            got = O.adam_ex_f32(p, g, m, v, x, step, LR, B1, B2, EPS, WD, **kw)
            for name, a, r, b in zip(("p", "m", "v", "vmax"), got, ref, bound):
                if a is None:
                    assert r is None and not amsgrad
                    continue
                err = (a.double() - r).abs()
                assert bool((err <= b).all()), (tag, step, name, (err / b.clamp_min(1e-300)).max().item())
                assert bool(torch.isfinite(b).all()) and bool((b >= 0).all())


def test_trajectory_bounds_chain_with_amsgrad_and_decay():
    """err= : ten fp32 steps fed their own outputs stay inside the accumulated bound"""
    p, g, m, v, x = O.warm_state(300, 9)
    cur32 = (p, m, v, x)
    cur64, err = (p.double(), m.double(), v.double(), x.double()), None
    gen = torch.Generator().manual_seed(10)
    for step in range(1, 11):
        g = torch.randn(300, generator=gen)
        lr_now = O.lr_ref(LR, step, **O.SCHEDULES["cosine"])
        kw = dict(decoupled=True, amsgrad=True, coef=0.5, lr_now=lr_now)
        cur64, err = O.adam_ex_ref(cur64[0], g, cur64[1], cur64[2], cur64[3], step, LR, B1, B2, EPS, WD, coef_rel=2 * R.U,
                                   err=err, **kw)
        cur32 = O.adam_ex_f32(cur32[0], g, cur32[1], cur32[2], cur32[3], step, LR, B1, B2, EPS, WD, **kw)
        for a, r, b in zip(cur32, cur64, err):
            assert bool(((a.double() - r).abs() <= b).all()), step


def test_constructors_validate_before_any_gpu_use():
    import pathnet_amd
    p = torch.nn.Parameter(torch.zeros(4))
    S = pathnet_amd.LRSchedule
    for kw in (dict(kind="linear"), dict(warmup_steps=-1), dict(warmup_steps=1.5), dict(start_factor=1.5),
               dict(start_factor=-0.1), dict(kind="step", gamma=0.5), dict(kind="step", step_size=0, gamma=0.5),
               dict(kind="step", step_size=3), dict(kind="step", step_size=3, gamma=0.0),
               dict(kind="exponential"), dict(kind="exponential", gamma=-0.5), dict(kind="exponential", gamma=math.inf),
               dict(kind="cosine"), dict(kind="cosine", t_max=0), dict(kind="cosine", t_max=5, lr_min=-1e-3)):
        with pytest.raises(ValueError):
            S(**kw)
    for cls in (pathnet_amd.Adam, pathnet_amd.AdamW):
        for kw in (dict(max_grad_norm=-1.0), dict(max_grad_norm=0.0), dict(max_grad_norm=float("nan")),
                   dict(schedule="cosine"), dict(lr=0.005, schedule=S("cosine", t_max=5, lr_min=0.01)),
                   dict(lr=-1.0), dict(weight_decay=-0.1)):
            with pytest.raises(ValueError):
                cls([p], **kw)
    with pytest.raises(ValueError):
        pathnet_amd.clip_grad_norm_([p], -1.0)
    # what is allowed: inf = the guard alone, lr_min == lr
    opt = pathnet_amd.AdamW([p], lr=0.005, max_grad_norm=math.inf, schedule=S("cosine", t_max=5, lr_min=R.f32(0.005)))
    assert opt.has_options and opt.defaults["weight_decay"] == 1e-2 and opt.decoupled_weight_decay
    assert not pathnet_amd.Adam([p]).has_options
    for kw in (dict(amsgrad=True), dict(decoupled_weight_decay=True), dict(max_grad_norm=1.0), dict(skip_nonfinite=True),
               dict(schedule=S())):
        assert pathnet_amd.Adam([p], **kw).has_options
    assert opt.last_lr is None and opt.last_grad_norm is None and opt.last_clip_coef is None and opt.skipped_steps is None


def test_options_refuse_cpu_parameters():
    import pathnet_amd
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="GPU"):
        pathnet_amd.AdamW([p], max_grad_norm=1.0).step()
    with pytest.raises(RuntimeError, match="GPU"):
        pathnet_amd.clip_grad_norm_([p], 1.0)
    assert torch.equal(p.detach(), torch.zeros(4)) and torch.equal(p.grad, torch.ones(4))


@pytest.mark.parametrize("decoupled", (False, True))
def test_state_dict_keys_and_round_trip_with_torch(decoupled):
    """the state a torch optimizer saved loads into ours (step back to an int, max_exp_avg_sq kept), and ours into torch's"""
    import pathnet_amd
    torch.manual_seed(6)
    q = torch.nn.Parameter(torch.randn(5))
    tcls, ocls = (torch.optim.AdamW, pathnet_amd.AdamW) if decoupled else (torch.optim.Adam, pathnet_amd.Adam)
    topt = tcls([q], lr=0.005, amsgrad=True)
    for _ in range(3):
        q.grad = torch.randn(5)
        topt.step()
    sd = topt.state_dict()
    ours = ocls([q], lr=0.005, amsgrad=True)
    ours.load_state_dict(sd)
    st = ours.state[q]
    assert set(st) == set(topt.state[q]) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}
    assert st["step"] == 3 and isinstance(st["step"], int)
    for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
        assert torch.equal(st[k], topt.state[q][k])
    back = ours.state_dict()
    assert set(back["state"][0]) == set(sd["state"][0])
    t2 = tcls([q], lr=0.005, amsgrad=True)
    t2.load_state_dict(back)
    for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
        assert torch.equal(t2.state[q][k], topt.state[q][k])
    assert float(t2.state[q]["step"]) == 3.0


def _const(text, pattern):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


def test_case_tables_straddle_the_dispatch_constants():
    with open(os.path.join(ROOT, "pathnet_amd", "csrc", "pn_optim.hip")) as f:
        src = f.read()
    with open(os.path.join(ROOT, "include", "pathnet_hip.h")) as f:
        header = f.read()
    chunk = int(_const(src, r"constexpr int OPT_CHUNK = (\d+);"))
    threads = int(_const(src, r"constexpr int OPT_THREADS = (\d+);"))
    cap = int(_const(src, r"constexpr int OPT_GRID_CAP = (\d+);"))
    max_tensors = int(_const(header, r"#define PN_ADAM_MAX_TENSORS (\d+)"))
    assert (O.OPT_CHUNK, O.OPT_THREADS, O.OPT_GRID_CAP, O.MAX_TENSORS) == (chunk, threads, cap, max_tensors)
    for kernel in ("grad_sumsq_kernel", "grad_scale_kernel", "adam_ex_kernel"):
        assert re.search(r"__launch_bounds__\(OPT_THREADS\) void %s" % kernel, src), kernel
    assert re.search(r"chunks < OPT_GRID_CAP \? chunks : OPT_GRID_CAP", src), "the grid cap's expression moved"
    counts = set(O.NORM_COUNTS)
    assert {1, threads - 1, threads, threads + 1, chunk - 1, chunk, chunk + 1, cap * chunk + 1} <= counts
    lengths = set(O.NORM_LIST_LENGTHS)
    assert {max_tensors - 1, max_tensors, max_tensors + 1, 2 * max_tensors + 1} <= lengths
    assert {c.index(0) for c in O.NORM_ZERO_POSITIONS} == {0, 1, 2}
    assert any(c > chunk for z in O.NORM_ZERO_POSITIONS for c in z)
    assert len(O.UPDATE_COMBOS) == 12 and set(O.CLIP_MODES) == {"none", "active", "inactive"}
    assert O.CLIP_MODES["active"] == 0.1 and O.CLIP_MODES["inactive"] == 10.0
    assert set(O.SCHEDULES) == {"constant", "step", "exponential", "cosine"}
    assert set(O.SCHEDULE_STEPS) == {1, 2, O.WARMUP, O.WARMUP + 1, O.T_MAX, O.T_MAX + 1, 10 ** 6}
    # the schedules' values at the late step still matter (nothing underflows to an easy 0)
    for name, s in O.SCHEDULES.items():
        assert O.lr_ref(LR, 10 ** 6, **s) > 1e-5, name
    # the running maximum of the element table lies on both sides of v
    p, g, m, v, x = O.elements_state()
    assert (x[v > 0] > v[v > 0]).any() and (x[v > 0] < v[v > 0]).any()
