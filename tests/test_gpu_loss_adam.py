"""The two launches that close every training step -- pn_cross_entropy and pn_adam_step / pn_adam_step_advance
(pn_train.hip) -- and the step-state advance (pn_context.hip), through the C ABI, against the plain fp64 references of
tests/optim_ref.py at the edges of their dispatch rules (the tables live there; tests/test_optim_host.py holds them to
the constants in the sources).

Cross entropy: up to CE_ONE_BLOCK_ROWS rows one workgroup of 1024 threads stores the loss in a fixed order; beyond, up to
256 workgroups of 256 threads (a grid-stride loop from 65537 rows on) add their parts with atomics behind a memset.
Bound: as close to fp64 as stock fp32 torch up to a factor 8, with the floor 2e-6 (optim_ref.ce_bounds).
Adam: every output element within the rounding bound optim_ref.adam_ref derives from the kernel's operations.
Every output lives inside a sentinel-filled allocation and must leave it as it was outside its own elements; the logits
sit inside a NaN-filled one (Guarded, test_gpu_node_gemm.py)."""
import ctypes

import pytest
import torch

import optim_ref as R
from test_gpu_node_gemm import SENT, Guarded

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _lib():
    from pathnet_amd import _lib as L
    return L


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------
# cross entropy
# ------------------------------------------------------------------------------------------------
class CeRun:
    """one pn_cross_entropy launch on guarded buffers -> .loss (float), .loss_bits (int), .g (cpu fp32 [rows, classes] or
    None), .clean (nothing outside the loss word and the [rows, classes] window was written)"""

    def __init__(self, x, t, want_grad=True, loss_fill=NAN):
        L = _lib()
        rows, classes = x.shape
        xs = Guarded((rows, classes), NAN, values=x.float().cuda())
        loss = Guarded((1, 1), SENT)
        loss.win.fill_(loss_fill)
        g = Guarded((rows, classes), SENT) if want_grad else None
        tt = t.to(torch.int64).cuda()
        L.check(L.load().pn_cross_entropy(xs.ptr(), tt.data_ptr(), rows, classes, loss.ptr(), g.ptr() if g else None,
                                          _stream()))
        torch.cuda.synchronize()
        lh = loss.host()
        self.loss = lh.values()[0, 0].item()
        self.loss_bits = lh.values().view(torch.int32)[0, 0].item()
        self.clean = lh.untouched_outside()
        self.g = None
        if g is not None:
            gh = g.host()
            self.g = gh.values().clone()
            self.clean = self.clean and gh.untouched_outside()


def _check_ce(tag, run, x, t, ref=None):
    """loss and gradient of a launch within optim_ref.ce_bounds; gradient rows sum to zero within the gradient's bound"""
    l64, g64, lb, gb = ref if ref is not None else R.ce_bounds(x, t)
    le = abs(run.loss - l64)
    line = "%s: loss err / bound = %.3g" % (tag, le / lb)
    ok = le <= lb
    if run.g is not None:
        assert torch.isfinite(run.g).all(), tag
        ge = (run.g.double() - g64).abs().max().item()
        se = run.g.double().sum(1).abs().max().item()
        line += ", grad err / bound = %.3g, row sum / bound = %.3g" % (ge / max(gb, 1e-300), se / max(gb, 1e-300))
        ok = ok and ge <= gb and se <= gb
    print(line)
    assert ok, line
    assert run.clean, "%s: wrote outside its outputs" % tag


def _ce_edge(rows, classes):
    torch.manual_seed(rows * 1000 + classes)
    x = torch.randn(rows, classes) * 3
    t = torch.randint(0, classes, (rows,))
    ref = R.ce_bounds(x, t)
    a = CeRun(x, t, True, NAN)
    b = CeRun(x, t, True, 1e30)
    c = CeRun(x, t, False, NAN)
    tag = "rows %d classes %d" % (rows, classes)
    _check_ce(tag + " (loss word NaN)", a, x, t, ref)
    _check_ce(tag + " (loss word 1e30)", b, x, t, ref)
    _check_ce(tag + " (no gradient)", c, x, t, ref)
    assert torch.equal(a.g, b.g), "%s: g_logits differs between two runs" % tag
    if rows <= R.CE_ONE_BLOCK_ROWS:         # one workgroup, fixed order: the same bits whatever else the launch writes
        assert a.loss_bits == b.loss_bits == c.loss_bits, tag


@pytest.mark.parametrize("rows", R.CE_ROWS)
def test_cross_entropy_row_edges(rows):
    _ce_edge(rows, R.ce_classes_for_rows(rows))


@pytest.mark.parametrize("classes", R.CE_CLASSES)
def test_cross_entropy_class_edges(classes):
    _ce_edge(33, classes)


@pytest.mark.parametrize("scale", R.CE_SCALES)
def test_cross_entropy_values_randn(scale):
    """logits randn x scale: the probabilities must not lose bits with the size of the logits"""
    torch.manual_seed(int(scale))
    x = torch.randn(2000, 7) * scale
    t = torch.randint(0, 7, (2000,))
    _check_ce("randn x %g" % scale, CeRun(x, t), x, t)


def test_cross_entropy_values_equal_logits():
    rows, classes = 40, 5
    x = torch.tensor([0.0, 5.0, -1e4, 1e4, 3e-3]).repeat(8)[:, None].expand(rows, classes).contiguous()
    t = torch.arange(rows) % classes
    run = CeRun(x, t)
    _check_ce("equal logits", run, x, t)
    scale = (torch.tensor(1.0) / torch.tensor(float(rows))).item()
    assert (run.g.double()[t[:, None] != torch.arange(classes)[None, :]] - 0.2 * scale).abs().max().item() <= 2e-6 * scale


def test_cross_entropy_values_one_dominant_logit():
    """one logit 200 above the rest: where it is the target the row's gradient is ~0; elsewhere the target's is exactly
    -1 / rows (its probability is 0 in fp32), the dominant class's ~ +1 / rows"""
    torch.manual_seed(4)
    rows, classes = 64, 6
    x = torch.randn(rows, classes)
    dom = torch.arange(rows) % classes
    x[torch.arange(rows), dom] += 200.0
    t = dom.clone()
    t[1::2] = (dom[1::2] + 1 + torch.arange(rows)[1::2] % (classes - 1)) % classes
    assert (t[1::2] != dom[1::2]).all() and (t[0::2] == dom[0::2]).all()
    run = CeRun(x, t)
    l64, g64, lb, gb = R.ce_bounds(x, t)
    _check_ce("dominant logit", run, x, t, (l64, g64, lb, gb))
    scale = (torch.tensor(1.0) / torch.tensor(float(rows))).item()          # 1.0f / (float)rows, as the entry point forms it
    assert run.g[0::2].abs().max().item() <= gb
    odd = torch.arange(1, rows, 2)
    assert (run.g[odd, t[odd]] == -scale).all()
    assert (run.g[odd, dom[odd]].double() - scale).abs().max().item() <= gb
    rest = torch.ones(rows, classes, dtype=torch.bool)
    rest[torch.arange(rows), t] = False
    rest[torch.arange(rows), dom] = False
    assert run.g[rest].abs().max().item() <= gb


def test_cross_entropy_values_minus_infinity():
    """-inf at non-target classes: a finite loss and exactly zero gradient there, as torch gives"""
    torch.manual_seed(5)
    rows, classes = 50, 7
    x = torch.randn(rows, classes) * 3
    t = torch.randint(0, classes, (rows,))
    hole = torch.zeros(rows, classes, dtype=torch.bool)
    for r in range(rows):
        for k in range(1 + r % 3):
            hole[r, (int(t[r]) + 1 + (r + 2 * k) % (classes - 1)) % classes] = True
    assert not hole[torch.arange(rows), t].any() and (hole.sum(1) < classes - 1).all()
    x[hole] = float("-inf")
    run = CeRun(x, t)
    _check_ce("-inf logits", run, x, t)
    assert run.loss == run.loss and abs(run.loss) < 1e3
    assert (run.g[hole] == 0).all()


def test_cross_entropy_values_one_class():
    x = torch.tensor([[0.0], [3.5], [-1e4], [2e5]]).repeat(9, 1)
    t = torch.zeros(36, dtype=torch.int64)
    run = CeRun(x, t)
    _check_ce("one class", run, x, t)
    assert run.loss == 0.0 and (run.g == 0).all()


def test_cross_entropy_values_subnormal_probabilities():
    """a spread of ~100 between logits: probabilities of e^-90 ... e^-100 are subnormal in fp32"""
    torch.manual_seed(6)
    rows, classes = 48, 4
    off = torch.tensor([0.0, -90.0, -95.0, -100.0])
    x = torch.randn(rows, classes) * 0.1
    for r in range(rows):
        x[r] += off.roll(r % classes)
    t = torch.arange(rows) // 2 % classes
    run = CeRun(x, t)
    _check_ce("subnormal probabilities", run, x, t)


@pytest.mark.parametrize("rows", (5, 1025, 33000))
@pytest.mark.parametrize("bad", ("classes", "minus_one"))
def test_cross_entropy_target_out_of_range(rows, bad):
    """A target of `classes` or -1 (an unlabelled node) in rows that are neither the first nor the last: the loss is NaN, the
    row's gradient exactly zero, every other row's gradient that of the same launch with a valid target there."""
    classes = 4
    torch.manual_seed(rows)
    x = torch.randn(rows, classes) * 3
    t = torch.randint(0, classes, (rows,))
    where = sorted({1, rows // 2, rows - 2})
    tb = t.clone()
    tb[where] = classes if bad == "classes" else -1
    good = CeRun(x, t)
    got = CeRun(x, tb)
    assert good.loss == good.loss
    assert got.loss != got.loss, "the loss must be NaN, got %r" % got.loss
    assert (got.g[where] == 0).all()
    keep = torch.ones(rows, dtype=torch.bool)
    keep[where] = False
    assert torch.equal(got.g[keep], good.g[keep]) and got.clean
    # the loss alone (no gradient asked for) is poisoned as well
    alone = CeRun(x, tb, want_grad=False)
    assert alone.loss != alone.loss and alone.clean


def test_cross_entropy_wrappers():
    """the Python wrappers: logits as a transposed view, int32 targets, an upstream gradient through the module form"""
    import pathnet_amd
    torch.manual_seed(7)
    rows, classes = 257, 5
    base = (torch.randn(classes, rows) * 100).cuda()
    xt = base.t().requires_grad_(True)
    assert not xt.is_contiguous()
    t = torch.randint(0, classes, (rows,))
    l64, g64, lb, gb = R.ce_bounds(base.t().cpu(), t)
    loss = pathnet_amd.cross_entropy(xt, t.to(torch.int32).cuda())
    loss.backward()
    assert abs(loss.item() - l64) <= lb
    ge = (xt.grad.cpu().double() - g64).abs().max().item()
    print("transposed view, int32 targets: grad err / bound = %.3g" % (ge / gb))
    assert ge <= gb
    xt.grad = None
    (pathnet_amd.CrossEntropyLoss()(xt, t.cuda()) * 3).backward()
    # (the multiply by the upstream 3 rounds once more: u * 3 max |g|)
    ge = (xt.grad.cpu().double() - 3 * g64).abs().max().item()
    bound3 = 3 * gb + 3 * R.U * g64.abs().max().item()
    print("module form * 3: grad err / bound = %.3g" % (ge / bound3))
    assert ge <= bound3


@pytest.mark.parametrize("bad", ("classes", "minus_one"))
def test_fused_step_target_out_of_range(bad):
    """forward_loss(..., fused=True) with an out-of-range target in a middle row, every PN_POOL_STEP / deterministic
    setting: the loss is NaN (the mistake cannot be missed), the logits and every parameter gradient stay finite (the
    row's d loss / d logits is zero)."""
    from test_gpu_pool_step import MODES, Case
    for variant in ("homo", "pagg"):
        case = Case(variant, S=60, W=5, H=32, C=4)
        ids, codes, sel, y = case.dev
        y = y.clone()
        y[case.S // 2] = case.C if bad == "classes" else -1
        case.dev = (ids, codes, sel, y)
        for name, knob, det in MODES:
            loss, out, grads = case.step(knob, det)
            assert loss != loss, (variant, name, loss)
            assert torch.isfinite(out).all(), (variant, name)
            for k, v in grads.items():
                assert torch.isfinite(v).all(), (variant, name, k)
            assert any(v.abs().max().item() > 0 for v in grads.values()), (variant, name)


# ------------------------------------------------------------------------------------------------
# Adam
# ------------------------------------------------------------------------------------------------
def device_state(adam_step, seed=0, epoch=0):
    """a pn_step_state in device memory"""
    s = seed - (1 << 64) if seed >= 1 << 63 else seed
    return torch.tensor([epoch, s, adam_step, 0], dtype=torch.int64, device="cuda")


def state_values(t):
    e, s, a, r = t.tolist()
    return {"epoch": e, "seed": s & R.MASK64, "adam_step": a}, r


class AdamTensors:
    """a list of (param, grad, exp_avg, exp_avg_sq) in guarded device allocations, their host copies beside them"""

    def __init__(self, host):
        self.host = [tuple(a.float().contiguous() for a in h) for h in host]
        self.dev = [tuple(Guarded((1, h[0].numel()), SENT, values=a) for a in h) for h in self.host]
        self.grad_before = [d[1].buf.clone() for d in self.dev]

    @classmethod
    def random(cls, counts, seed):
        gen = torch.Generator().manual_seed(seed)
        host = []
        for n in counts:
            host.append((torch.randn(n, generator=gen), torch.randn(n, generator=gen),
                         0.1 * torch.randn(n, generator=gen), (0.1 * torch.randn(n, generator=gen)) ** 2))
        return cls(host)

    def launch(self, hyper, step=1, state=None, advance=False):
        L = _lib()
        lib = L.load()
        lr, (b1, b2), eps, wd = hyper
        n = len(self.dev)
        arr = (L.AdamTensor * max(n, 1))()
        for i, (p, g, m, v) in enumerate(self.dev):
            arr[i] = L.AdamTensor(p.ptr(), g.ptr(), m.ptr(), v.ptr(), p.cols)
        sp = ctypes.c_void_p(state.data_ptr()) if state is not None else None
        if advance:
            L.check(lib.pn_adam_step_advance(arr if n else None, n, lr, b1, b2, eps, wd, sp, _stream()))
        else:
            L.check(lib.pn_adam_step(arr if n else None, n, lr, b1, b2, eps, wd, step, sp, _stream()))
        torch.cuda.synchronize()

    def results(self):
        """[(p, m, v)] on the host; asserts that nothing outside `count` moved and that the gradients are untouched"""
        out = []
        for i, (p, g, m, v) in enumerate(self.dev):
            hp, hm, hv = p.host(), m.host(), v.host()
            assert hp.untouched_outside() and hm.untouched_outside() and hv.untouched_outside(), "tensor %d: wrote past count" % i
            assert torch.equal(g.buf, self.grad_before[i]), "tensor %d: the gradient was written" % i
            out.append((hp.values()[0].clone(), hm.values()[0].clone(), hv.values()[0].clone()))
        return out

    def check(self, tag, hyper, step):
        """every element of every output within adam_ref's bound -> (results, worst err / bound)"""
        lr, (b1, b2), eps, wd = hyper
        res = self.results()
        worst = 0.0
        for i, (h, got) in enumerate(zip(self.host, res)):
            ref, bounds = R.adam_ref(h[0], h[1], h[2], h[3], step, lr, b1, b2, eps, wd)
            for name, a, r, b in zip("pmv", got, ref, bounds):
                assert torch.isfinite(a).all(), (tag, i, name)
                err = (a.double() - r).abs()
                if err.numel():
                    worst = max(worst, (err / b.clamp_min(1e-300)).max().item())
                assert bool((err <= b).all()), "%s: tensor %d %s' off by %.3g of its bound" % (
                    tag, i, name, (err / b.clamp_min(1e-300)).max().item())
        print("%s: worst err / bound = %.3g" % (tag, worst))
        return res, worst


@pytest.mark.parametrize("name", sorted(R.ADAM_HYPER))
def test_adam_single_step_from_arbitrary_state(name):
    """one update at step counts from 1 to 2^31 - 1, the count given by the host and read from a device pn_step_state"""
    hyper = R.ADAM_HYPER[name]
    lr, (b1, b2), eps, wd = hyper
    p, g, m, v = R.adam_elements()
    still = (g == 0) & (m == 0) & (v == 0) & ((p == 0) | torch.tensor(wd == 0.0))
    assert still.any()
    for step in R.ADAM_STEPS:
        host = AdamTensors([(p, g, m, v)])
        host.launch(hyper, step=step)
        (hp, hm, hv), = host.check("%s step %d (host count)" % (name, step), hyper, step)[0]
        dev = AdamTensors([(p, g, m, v)])
        state = device_state(step, seed=5, epoch=9)
        dev.launch(hyper, step=1, state=state)
        (dp, dm, dv), = dev.check("%s step %d (device count)" % (name, step), hyper, step)[0]
        assert state_values(state) == ({"epoch": 9, "seed": 5, "adam_step": step}, 0)       # pn_adam_step moves nothing
        # g == 0 with m == v == 0 (and no decay pulling on it): the parameter does not move
        for q in (hp, dp):
            assert torch.equal(q[still], p[still])
        # the two launches agree within the sum of their bounds (pow and squaring differ in the last bits of a double)
        bounds = R.adam_ref(p, g, m, v, step, lr, b1, b2, eps, wd)[1]
        for a, b, e in zip((hp, hm, hv), (dp, dm, dv), bounds):
            assert bool(((a.double() - b.double()).abs() <= 2 * e).all())


@pytest.mark.parametrize("count", R.ADAM_COUNTS)
def test_adam_element_count_edges(count):
    hyper = R.ADAM_HYPER["recipe"]
    ts = AdamTensors.random([count], seed=count)
    ts.launch(hyper, step=3)
    ts.check("count %d" % count, hyper, 3)


@pytest.mark.parametrize("n", R.ADAM_LIST_LENGTHS)
def test_adam_tensor_count_edges(n):
    hyper = R.ADAM_HYPER["recipe"]
    ts = AdamTensors.random([17] * n, seed=n)
    ts.launch(hyper, step=4)
    ts.check("%d tensors" % n, hyper, 4)


@pytest.mark.parametrize("counts", ((0, 17, 2049), (17, 0, 2049), (17, 2049, 0)))
def test_adam_zero_element_tensor_in_a_list(counts):
    hyper = R.ADAM_HYPER["recipe"]
    ts = AdamTensors.random(list(counts), seed=sum(c * (i + 1) for i, c in enumerate(counts)))
    ts.launch(hyper, step=2)
    ts.check("counts %r" % (counts,), hyper, 2)


def test_adam_advance_when_the_last_launch_is_empty():
    """33 tensors, the 33rd empty, through pn_adam_step_advance: the second launch of the step has no elements, and the
    state still moves on exactly once (adam_advance_only_kernel); the update itself used the count before the advance"""
    hyper = R.ADAM_HYPER["recipe"]
    ts = AdamTensors.random([17] * 32 + [0], seed=33)
    state = device_state(7, seed=0xFEDCBA9876543210, epoch=41)
    before, _ = state_values(state)
    ts.launch(hyper, state=state, advance=True)
    ts.check("33 tensors, the last empty", hyper, 7)
    after, reserved = state_values(state)
    assert after == R.splitmix_advance(before) and reserved == 0


def test_adam_advance_with_elements_in_the_last_launch():
    """the ticket path: 33 tensors of which the 33rd spans three workgroups; one advance, the ticket word back at zero"""
    hyper = R.ADAM_HYPER["recipe"]
    ts = AdamTensors.random([17] * 32 + [4097], seed=34)
    state = device_state(3, seed=123, epoch=0)
    before, _ = state_values(state)
    ts.launch(hyper, state=state, advance=True)
    ts.check("33 tensors, the last of 4097", hyper, 3)
    after, reserved = state_values(state)
    assert after == R.splitmix_advance(before) and reserved == 0


def test_adam_advance_without_tensors():
    state = device_state(1, seed=99, epoch=-1)
    before, _ = state_values(state)
    AdamTensors([]).launch(R.ADAM_HYPER["recipe"], state=state, advance=True)
    after, reserved = state_values(state)
    assert after == R.splitmix_advance(before) and reserved == 0


TRAJECTORY_SHAPES = [(128, 1433), (128,), (512, 128), (7, 256), (1,), (3, 5, 7)] + [(17,)] * 40


@pytest.fixture(scope="module")
def trajectory():
    """the configuration of test_adam_matches_torch_optim_adam, every parameter given a gradient at every step:
    (initial parameters, gradients per step, torch.optim.Adam's float64 result) -- computed once, never modified"""
    gen = torch.Generator().manual_seed(3)
    init = [torch.randn(*s, generator=gen) for s in TRAJECTORY_SHAPES]
    grads = [[torch.randn(*s, generator=gen) for s in TRAJECTORY_SHAPES] for _ in range(25)]
    ref = [torch.nn.Parameter(p.double().clone()) for p in init]
    opt = torch.optim.Adam(ref, lr=0.005, weight_decay=0.0005)
    for gs in grads:
        for q, g in zip(ref, gs):
            q.grad = g.double()
        opt.step()
    return init, grads, [q.detach().clone() for q in ref]


@pytest.mark.parametrize("auto", (False, True))
def test_adam_trajectory_with_the_device_step_count(trajectory, auto):
    """25 steps whose bias corrections are formed on the device from StepState's count, against torch.optim.Adam in
    float64.  With advance_in_adam the 25th update leaves the state at the count of the step that would follow."""
    import pathnet_amd
    init, grads, want = trajectory
    ps = [torch.nn.Parameter(p.clone().cuda()) for p in init]
    st = pathnet_amd.StepState("cuda", seed=1, first_epoch=0, advance_in_adam=auto)
    opt = pathnet_amd.Adam(ps, lr=0.005, weight_decay=0.0005, step_state=st)
    for gs in grads:
        st.advance()
        for p, g in zip(ps, gs):
            p.grad = g.cuda()
        opt.step()
        count_of_this_step = st.values()["adam_step"] - (1 if auto else 0)
    torch.cuda.synchronize()
    assert count_of_this_step == 25 and st.values()["adam_step"] == (26 if auto else 25)
    worst = max((p.detach().cpu().double() - q).abs().max().item() for p, q in zip(ps, want))
    print("trajectory (advance_in_adam=%s): max |p - p64| = %.3g (bound 2e-6)" % (auto, worst))
    assert worst < 2e-6
    assert int(st.t[3].item()) == 0


def test_adam_replayed_in_a_graph_follows_the_reference():
    """`st.advance(); opt.step()` captured alone (a linear chain) and replayed five times with refilled gradients: the
    parameters equal adam_ref iterated at steps 2 .. 6 within the bounds added up along the trajectory."""
    import pathnet_amd
    hyper = R.ADAM_HYPER["recipe"]
    lr, (b1, b2), eps, wd = hyper
    gen = torch.Generator().manual_seed(8)
    shapes = [(300,), (5, 7), (1,)]
    init = [torch.randn(*s, generator=gen) for s in shapes]
    grads = [[torch.randn(*s, generator=gen) for s in shapes] for _ in range(6)]
    ps = [torch.nn.Parameter(p.clone().cuda()) for p in init]
    static = [g.clone().cuda() for g in grads[0]]
    for p, g in zip(ps, static):
        p.grad = g
    st = pathnet_amd.StepState("cuda", seed=2)
    opt = pathnet_amd.Adam(ps, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, step_state=st)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):           # warm-up = step 1 (creates the optimizer state)
        st.advance()
        opt.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st.advance()
        opt.step()
    # (capture launches nothing: the state is still at step 1)
    assert st.values()["adam_step"] == 1
    for k in range(1, 6):
        for s, g in zip(static, grads[k]):
            s.copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    assert st.values()["adam_step"] == 6
    worst = 0.0
    for i, p0 in enumerate(init):
        cur, err = (p0.double(), torch.zeros_like(p0).double(), torch.zeros_like(p0).double()), None
        for k in range(6):
            cur, err = R.adam_ref(cur[0], grads[k][i], cur[1], cur[2], k + 1, lr, b1, b2, eps, wd, err=err)
        e = (ps[i].detach().cpu().double() - cur[0]).abs()
        worst = max(worst, (e / err[0]).max().item())
        assert bool((e <= err[0]).all()), (i, (e / err[0]).max().item())
        m_e = (opt.state[ps[i]]["exp_avg"].cpu().double() - cur[1]).abs()
        v_e = (opt.state[ps[i]]["exp_avg_sq"].cpu().double() - cur[2]).abs()
        assert bool((m_e <= err[1]).all()) and bool((v_e <= err[2]).all()), i
    print("five replays: worst err / summed bound = %.3g" % worst)


# ------------------------------------------------------------------------------------------------
# step state
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,first_epoch", R.STATE_SEEDS)
def test_step_state_follows_splitmix64(seed, first_epoch):
    """both copies of the advance -- step_state_advance_kernel through advance(), advance_step_state through Adam's last
    launch -- against the Python integers of optim_ref.splitmix_advance, exactly"""
    import pathnet_amd
    want = {"epoch": first_epoch - 1, "seed": seed, "adam_step": 0}
    st = pathnet_amd.StepState("cuda", seed=seed, first_epoch=first_epoch)
    assert st.values() == want
    for _ in range(5):
        st.advance()
        want = R.splitmix_advance(want)
        assert st.values() == want
    want = {"epoch": first_epoch - 1, "seed": seed, "adam_step": 0}
    st = pathnet_amd.StepState("cuda", seed=seed, first_epoch=first_epoch, advance_in_adam=True)
    p = torch.nn.Parameter(torch.ones(5000, device="cuda"))      # three workgroups take tickets
    opt = pathnet_amd.Adam([p], lr=0.01, step_state=st)
    st.advance()
    want = R.splitmix_advance(want)
    assert st.values() == want
    for _ in range(5):
        p.grad = torch.ones_like(p)
        opt.step()
        want = R.splitmix_advance(want)
        assert st.values() == want
        st.advance()                        # launches nothing: the update has moved the state already
        assert st.values() == want
    assert int(st.t[3].item()) == 0
