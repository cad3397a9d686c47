"""Host-side behaviour of the loss / optimizer wrappers (no GPU): they refuse CPU tensors instead of falling back.
Also on the CPU: the fp64 references of tests/optim_ref.py against torch's own float64 implementations, and the case
tables of tests/test_gpu_loss_adam.py against the dispatch constants of the sources they are meant to straddle."""
import os
import re

import pytest
import torch

import optim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adam_refuses_cpu_parameters():
    import pathnet_amd
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    opt = pathnet_amd.Adam([p], lr=0.01, weight_decay=0.1)
    with pytest.raises(RuntimeError, match="GPU"):
        opt.step()
    assert torch.equal(p.detach(), torch.zeros(4))          # untouched


def test_adam_validates_hyper_parameters():
    import pathnet_amd
    p = torch.nn.Parameter(torch.zeros(4))
    for kw in (dict(lr=-1.0), dict(eps=-1e-8), dict(weight_decay=-0.1), dict(betas=(1.0, 0.999))):
        with pytest.raises(ValueError):
            pathnet_amd.Adam([p], **kw)


def test_cross_entropy_refuses_cpu_logits():
    import pathnet_amd
    with pytest.raises(RuntimeError, match="GPU"):
        pathnet_amd.cross_entropy(torch.zeros(3, 2), torch.zeros(3, dtype=torch.long))


@pytest.mark.parametrize("name", sorted(R.ADAM_HYPER))
def test_adam_ref_equals_torch_adam_in_float64(name):
    """ten steps from zero state, torch.optim.Adam constructed with the same float32-rounded hyper-parameters"""
    lr, betas, eps, wd = R.ADAM_HYPER[name]
    torch.manual_seed(1)
    shapes = [(37, 5), (1,), (300,)]
    ref = [torch.nn.Parameter(torch.randn(*s, dtype=torch.float64)) for s in shapes]
    opt = torch.optim.Adam(ref, lr=R.f32(lr), betas=(R.f32(betas[0]), R.f32(betas[1])), eps=R.f32(eps),
                           weight_decay=R.f32(wd), foreach=False)
    ours = [(q.detach().clone(), torch.zeros_like(q), torch.zeros_like(q)) for q in ref]
    for step in range(1, 11):
        for i, q in enumerate(ref):
            g = torch.randn(*q.shape, dtype=torch.float64)
            q.grad = g.clone()
            p, m, v = ours[i]
            ours[i] = R.adam_ref(p, g, m, v, step, lr, betas[0], betas[1], eps, wd)[0]
        opt.step()
    for q, (p, m, v) in zip(ref, ours):
        st = opt.state[q]
        for got, want in ((p, q.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
            assert ((got - want).abs() <= 1e-14 * want.abs().max()).all()
        assert ((p - q.detach()).abs() <= 1e-14 * q.detach().abs()).all()       # the parameters element by element


def test_adam_ref_bounds_are_roundings_not_slack():
    """the bound of every output is a few u of the terms it is made of -- finite, and zero where nothing can move"""
    p, g, m, v = R.adam_elements()
    lr, betas, eps, wd = R.ADAM_HYPER["wd0"]
    (p1, m1, v1), (ep, em, ev) = R.adam_ref(p, g, m, v, 10, lr, betas[0], betas[1], eps, wd)
    for e in (ep, em, ev):
        assert torch.isfinite(e).all() and (e >= 0).all()
    still = (g == 0) & (m == 0) & (v == 0)
    assert still.any() and (p1[still] == p[still].double()).all() and (em[still] == 0).all() and (ev[still] == 0).all()
    assert (ep[still] <= 1.001 * R.U * p1[still].abs()).all()
    assert (em <= 16 * R.U * (m1.abs() + m.double().abs() + g.double().abs())).all()
    assert (ev <= 16 * R.U * v1).all()


def test_cross_entropy_ref_equals_torch_in_float64():
    torch.manual_seed(2)
    for rows, classes, scale in ((1, 1, 1.0), (33, 7, 3.0), (200, 5, 1e3), (64, 300, 1e4)):
        x = torch.randn(rows, classes, dtype=torch.float64) * scale
        t = torch.randint(0, classes, (rows,))
        if classes >= 5:            # -inf at non-target classes of some rows
            for r in range(0, rows, 3):
                x[r, (int(t[r]) + 1 + r % (classes - 1)) % classes] = float("-inf")
                assert x[r, t[r]] > float("-inf")
        xr = x.clone().requires_grad_(True)
        want = torch.nn.functional.cross_entropy(xr, t)
        want.backward()
        l64, g64, l32, g32 = R.cross_entropy_ref(x, t)
        assert abs(l64 - want.item()) <= 1e-14 * max(1.0, abs(want.item()))
        assert (g64 - xr.grad).abs().max().item() <= 1e-15
        assert (g64[x == float("-inf")] == 0).all()
        # an explicit scale: the sum times it
        l64s, g64s, _, _ = R.cross_entropy_ref(x, t, scale=0.25)
        assert abs(l64s - 0.25 * rows * want.item()) <= 1e-13 * max(1.0, abs(l64s))
        assert (g64s - 0.25 * rows * xr.grad).abs().max().item() <= 1e-14
        # the yardstick is fp32's answer to the same question: close to, and not the same as, the fp64 one
        assert abs(l32 - l64) <= 1e-5 * max(1.0, abs(l64)) and (g32 - g64).abs().max().item() <= 1e-6


def test_splitmix_advance_is_splitmix64():
    """the published test vector of splitmix64: seed 1234567 -> 6457827717110365317, 3203168211198807973"""
    s = {"epoch": -1, "seed": 1234567, "adam_step": 0}
    s1 = R.splitmix_advance(s)
    assert s1 == {"epoch": 0, "seed": 6457827717110365317, "adam_step": 1}
    # the kernels keep the MIXED value as the next state (not the Weyl sequence): the second value differs from the stream's
    s2 = R.splitmix_advance(s1)
    assert s2["epoch"] == 1 and s2["adam_step"] == 2 and s2["seed"] != 3203168211198807973 and 0 <= s2["seed"] < 1 << 64
    # one of the GPU test's seeds reaches a value with the top bit set
    tops = []
    for seed, e in R.STATE_SEEDS:
        st = {"epoch": e - 1, "seed": seed, "adam_step": 0}
        for _ in range(10):
            st = R.splitmix_advance(st)
            tops.append(st["seed"] >> 63)
    assert 1 in tops and 0 in tops
    assert len(R.STATE_SEEDS) >= 3


def _source(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _const(text, pattern):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


def test_case_tables_straddle_the_dispatch_constants():
    """The constants are read out of the sources: when one changes, this test fails instead of the GPU tests silently
    leaving the edge."""
    train = _source("pathnet_amd", "csrc", "pn_train.hip")
    header = _source("include", "pathnet_hip.h")
    one_block = int(_const(train, r"constexpr int CE_ONE_BLOCK_ROWS = (\d+);"))
    chunk = int(_const(train, r"constexpr int ADAM_CHUNK = (\d+);"))
    max_tensors = int(_const(header, r"#define PN_ADAM_MAX_TENSORS (\d+)"))
    # the launch shape past one workgroup: `threads` rows per block, at most `cap` blocks
    m = re.search(r"const int threads = rows <= CE_ONE_BLOCK_ROWS \? (\d+) : (\d+);", train)
    assert m, "cross entropy: the thread counts moved"
    wide_threads, threads = int(m.group(1)), int(m.group(2))
    m = re.search(r"const int blocks = rows <= CE_ONE_BLOCK_ROWS \? 1 : \(\(rows \+ (\d+)\) / (\d+) < (\d+) \? "
                  r"\(rows \+ (\d+)\) / (\d+) : (\d+)\);", train)
    assert m, "cross entropy: the block count's expression moved"
    a, b, cap, c, d, cap2 = (int(v) for v in m.groups())
    assert a == c == threads - 1 and b == d == threads and cap == cap2
    adam_threads = int(_const(train, r"dim3\(blocks\), dim3\((\d+)\), 0, stream, a\);"))
    assert re.search(r"__launch_bounds__\(%d\) void adam_kernel" % adam_threads, train)

    assert R.CE_ONE_BLOCK_ROWS == one_block
    rows = set(R.CE_ROWS)
    assert {1, 63, 64, 65} <= rows                                          # one wavefront
    assert {wide_threads - 1, wide_threads, wide_threads + 1} <= rows       # one workgroup's threads: a second row per thread
    assert {one_block - 1, one_block, one_block + 1} <= rows                # store -> memset + atomics
    grid = cap * threads
    assert {grid - 1, grid, grid + 1} <= rows                               # the block cap, the first grid-stride wrap
    assert one_block + 1 > threads                                          # (the multi-workgroup side has several blocks)
    assert {ceil(r, threads) for r in rows if r > one_block} >= {ceil(one_block + 1, threads), cap, cap + 1}
    assert {R.ce_classes_for_rows(r) for r in R.CE_ROWS} == {2, 3}
    assert set(R.CE_CLASSES) >= {1, 2, 63, 64, 65, 300}
    assert set(R.CE_SCALES) == {3.0, 100.0, 1e3, 1e4}

    counts = set(R.ADAM_COUNTS)
    assert {1, adam_threads - 1, adam_threads, adam_threads + 1} <= counts
    assert {chunk - 1, chunk, chunk + 1, 2 * chunk + 1} <= counts
    lengths = set(R.ADAM_LIST_LENGTHS)
    assert {max_tensors - 1, max_tensors, max_tensors + 1, 2 * max_tensors, 2 * max_tensors + 1} <= lengths
    assert set(R.ADAM_STEPS) == {1, 2, 10, 1000, 10 ** 6, 2 ** 31 - 1}
    assert set(R.ADAM_HYPER) == {"recipe", "wd0", "eps1e-3", "beta1_0"} and R.ADAM_HYPER["beta1_0"][1][0] == 0.0

    # the element classes of the single-step test
    p, g, m_, v = R.adam_elements()
    ag = g.abs()
    for e in range(-12, 5):
        assert ((ag > 0.5 * 10.0 ** e) & (ag < 2 * 10.0 ** e)).any(), e
    assert ((g == 0) & (m_ == 0) & (v == 0)).any() and ((g == 0) & (m_ != 0) & (v != 0)).any()
    for e in range(-6, 4):
        assert ((p.abs() > 0.5 * 10.0 ** e) & (p.abs() < 2 * 10.0 ** e)).any(), e
    assert ((v > 0) & (v < 1e-20) & (m_.abs() >= 0.1)).any()
    assert (v[v > 0] >= 1e-30).all()            # nothing subnormal


def ceil(a, b):
    return -(-a // b)
