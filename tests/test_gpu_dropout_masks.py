"""The built-in dropout masks, bit for bit, against the Philox reference of tests/dropout_ref.py.

Every kernel that draws a mask (dropout4 / dropout1, pathnet_amd/csrc/pn_kernels.h) is read out through the module
surface with the probe parameters of tests/dropout_probes.py -- an output is non-zero exactly where a bit is kept; the
constructions are proved on the CPU oracle in tests/test_dropout_host.py -- and the decoded bits must EQUAL the reference
at every position; there is no tolerance.  What draws, and what reads it here:

  seq_fwdh_kernel / seq_fwd3_kernel   (pn_seqh.hip / pn_seq3.hip; seq_math f16x2 / bf16x3, H <= 256)   the paths' final
  seq_reduce_kernel (mean / sum), gen_mask (256 < H <= 1024)                                           states of encode()
  seq_bwdh_kernel / seq_bwd3_kernel and the generic / reducing backward (saved keep bytes, or drawn
  again when a micro-batch is re-run)                                                                   X.grad, row by row
  the pooling kernels of pn_pool.hip (stream 2), forward, backward and the fused step's                fc2.weight.grad, X.grad

over P = S W in {1, 33, 65}, L in {1, 4}, p in {0.1, 0.5, 0.9}, the seeds 0, one drawn through torch.manual_seed and
2^62 - 1, H in {32, 96, 128, 256} in both seq_math modes, H = 100 (the counters run on the padded 128), H = 288, every
cell and class, deterministic mode on and off, micro-batches, group_slice, batch_position and a StepState.  Beside the
bits, the built-in-dropout cases that tests/test_gpu_bwdh_edges.py and tests/test_gpu_seqh.py hold to the bf16 x 3 kernels
are held to the CPU oracle under the reconstructed masks, and so is the fused step.

Not covered: counters beyond 2^32 (P L H / 4 > 2^32 is far past a seconds-long test; the 64-bit counter words are
exercised in tests/test_dropout_host.py only) and the runners of pathnet_amd.dist."""
import functools

import numpy as np
import pytest
import torch

import dropout_probes as dp
import dropout_ref as dr
from gradcheck import GRAD_REL, NOISE, assert_grads_close, grad_report
from optim_ref import cross_entropy_ref, splitmix_advance
from oracle import pagg_oracle as po

pytestmark = pytest.mark.gpu

N, C = dp.N, 16
SEED_KINDS = ("zero", "torch", "max")
TORCH_SEED = 5


@functools.lru_cache(maxsize=None)
def _masks(seed, p, L, S, W, H):
    return dr.module_masks(seed, p, L, S, W, H)


def _seed_of(kind):
    return {"zero": 0, "torch": dr.module_seed(TORCH_SEED), "max": 2 ** 62 - 1}[kind]


def _module(variant, cell, H, L, p, math="f16x2", det=False):
    import pathnet_amd
    if variant == "pagg":
        m = pathnet_amd.PAGG(H, H, C, N, dropout=p, cell=cell)
    else:
        m = {"homo": pathnet_amd.PathNet_homo, "hetero": pathnet_amd.PathNet}[variant](H, H, C, L, dropout=p, cell=cell)
    m = m.cuda().train()
    m.seq_math, m.deterministic = math, det
    return m


def _load(m, sd):
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def _index_args(sel, ids, codes, W, L):
    S = len(sel)
    mask = np.zeros(N, bool)
    mask[sel] = True
    return (torch.as_tensor(ids.reshape(S, W * L).astype(np.int64)), W, L, mask, torch.as_tensor(codes.astype(np.int64)), None)


def _encode(m, X, sel, ids, codes, W, L, kind, **kw):
    """encode() under the seed of `kind`: given explicitly, or drawn by the module from torch's generator"""
    if kind == "torch":
        torch.manual_seed(TORCH_SEED)
        return m.encode(X, *_index_args(sel, ids, codes, W, L), path_state=True, **kw)
    return m.encode(X, *_index_args(sel, ids, codes, W, L), path_state=True, seed=_seed_of(kind), **kw)


def _forward_bits(m, case, X, sel, ids, codes, kind, begin=0, count=None, bits=None):
    """the sequence mask as the forward applied it: one run per step (one run in all for mean / sum)"""
    variant, cell, H, S, W, L, p = case
    bits = torch.zeros(L, S * W, H, dtype=torch.bool) if bits is None else bits
    slot = dp.slots(variant, S, W, begin, count)
    kw = {} if count is None else {"group_slice": (begin, count)}
    if cell in dp.REDUCING:
        _load(m, dp.params(variant, cell, H, L, C, dp.amp_powers(L)))
        dp.put_sum_bits(bits, _encode(m, X, sel, ids, codes, W, L, kind, **kw).path_state, slot, L, cell == "mean")
    else:
        for t in range(L):
            _load(m, dp.params(variant, cell, H, L, C, dp.amp_one_step(p, L, t)))
            dp.put_forward_bits(bits, t, _encode(m, X, sel, ids, codes, W, L, kind, **kw).path_state, slot)
    return bits


def _backward_x_grad(m, case, sel, ids, codes, kind, **kw):
    """X.grad of a loss over the pooled half of the embedding, every step active"""
    variant, cell, H, S, W, L, p = case
    amp = dp.amp_powers(L) if cell in dp.REDUCING else dp.amp_every_step(p, L)
    _load(m, dp.params(variant, cell, H, L, C, amp))
    X = torch.zeros(N, H, device="cuda", requires_grad=True)
    enc = _encode(m, X, sel, ids, codes, W, L, kind, **kw)
    enc.embedding[:, H:].sum().backward()
    torch.cuda.synchronize()
    return X.grad


def _classifier_read(m, case, run):
    """-> (bits [S, 2H] from fc2.weight.grad, X.grad of every pass): run(G) -> logits of one forward under the seed"""
    variant, cell, H, S, W, L, p = case
    _load(m, dp.params(variant, cell, H, L, C, dp.amp_every_step(p, L), cell_bias=1.0))
    grads, xg = [], []
    for k in range(-(-S // C)):
        m.zero_grad(set_to_none=True)
        X = torch.zeros(N, H, device="cuda", requires_grad=True)
        out = run(X)
        (out * dp.one_hot_pass(S, C, k).cuda()).sum().backward()
        grads.append(m.fc2.weight.grad.detach().clone())
        xg.append(X.grad.detach().cpu())
    return dp.classifier_bits(grads, S, C), xg


GPU_CASES = []
for _i, _c in enumerate(dp.PROBE_CASES):
    _fused = _c[2] <= 256 and _c[1] not in dp.REDUCING
    for _j, _math in enumerate(("f16x2", "bf16x3") if _fused else ("f16x2",)):
        GPU_CASES.append(pytest.param(_c, _math, SEED_KINDS[(_i + _j) % 3], bool((_i + _j) & 1),
                                      id="%s-%s-%s-det%d" % (dp.case_id(_c), _math, SEED_KINDS[(_i + _j) % 3], (_i + _j) & 1)))


@pytest.mark.parametrize("case,math,kind,det", GPU_CASES)
def test_forward_sequence_mask_bits(case, math, kind, det):
    variant, cell, H, S, W, L, p = case
    m = _module(variant, cell, H, L, p, math, det)
    sel, ids, codes = dp.paths(S, W, L, seed=3)
    bits = _forward_bits(m, case, torch.zeros(N, H, device="cuda"), sel, ids, codes, kind)
    assert torch.equal(bits, _masks(_seed_of(kind), p, L, S, W, H)[0] != 0)


@pytest.mark.parametrize("case,math,kind,det", GPU_CASES)
def test_backward_sequence_mask_bits(case, math, kind, det):
    variant, cell, H, S, W, L, p = case
    m = _module(variant, cell, H, L, p, math, det)
    sel, ids, codes = dp.paths(S, W, L, seed=3)
    xg = _backward_x_grad(m, case, sel, ids, codes, kind)
    node = po.plan(variant, ids, codes, S, W, L)[0]
    assert torch.equal(dp.backward_bits(xg, node), _masks(_seed_of(kind), p, L, S, W, H)[0] != 0)
    others = np.setdiff1d(np.arange(N), node.reshape(-1))
    assert float(xg[torch.as_tensor(others).cuda()].abs().max()) == 0.0


@pytest.mark.parametrize("case", [c for c in dp.PROBE_CASES if c[1] not in dp.REDUCING], ids=dp.case_id)
def test_classifier_mask_bits(case):
    """forward() with the seed taken through torch.manual_seed; the backward's own draw shows in X.grad"""
    variant, cell, H, S, W, L, p = case
    m = _module(variant, cell, H, L, p)
    sel, ids, codes = dp.paths(S, W, L, seed=3)
    args = _index_args(sel, ids, codes, W, L)
    outs = []

    def run(X):
        torch.manual_seed(TORCH_SEED)
        outs.append(m(X, *args))
        return outs[-1]
    bits, xg = _classifier_read(m, case, run)
    seed = dr.module_seed(TORCH_SEED)
    ms, mc = _masks(seed, p, L, S, W, H)
    # the embedding the classifier's mask multiplies is positive everywhere: encode() of the same call, same logits
    enc = m.encode(torch.zeros(N, H, device="cuda"), *args, seed=seed)
    assert torch.equal(enc.logits.detach(), outs[-1].detach()) and float(enc.embedding.detach().min()) > 0.0
    assert torch.equal(bits, mc != 0)
    ego, joint = dp.joint_bits(xg, sel, po.plan(variant, ids, codes, S, W, L)[0], S, W, C, variant)
    assert torch.equal(ego, mc[:, :H] != 0)
    group = dp.group_of(variant, S, W)
    assert torch.equal(joint, (ms != 0) & (mc[:, H:] != 0)[torch.as_tensor(group)][None])


@pytest.mark.parametrize("case", [c for c in dp.PROBE_CASES if c[0] == "homo" and c[1] not in dp.REDUCING], ids=dp.case_id)
def test_merged_step0_rows_count_the_kept_bits(case):
    """ids[:, :, 0] = sel: the homo plan merges a node's W step-0 rows, and X.grad on the shared row counts the kept bits
    among W equal contributions; the size of one contribution is the oracle's"""
    variant, cell, H, S, W, L, p = case
    m = _module(variant, cell, H, L, p)
    sel, ids, codes = dp.paths(S, W, L, seed=3, ego_first=True)
    seed = 2 ** 62 - 1
    ms, mc = _masks(seed, p, L, S, W, H)
    sd = dp.params(variant, cell, H, L, C, dp.amp_one_step(p, L, 0))
    want = (ms[0] != 0).view(S, W, H).sum(dim=1)
    r = dp.oracle_run(variant, cell, sd, torch.zeros(N, H), sel, ids, codes, W, L, ms, mc, loss=dp.pooled_loss(H))
    g = r["grads"]["X"][sel]
    unit = float((g[want > 0] / want[want > 0]).median()) if bool((want > 0).any()) else 1.0
    _load(m, sd)
    X = torch.zeros(N, H, device="cuda", requires_grad=True)
    enc = m.encode(X, *_index_args(sel, ids, codes, W, L), seed=seed)
    enc.embedding[:, H:].sum().backward()
    assert torch.equal(dp.merged_counts(X.grad[torch.as_tensor(sel).cuda()], unit), want)


MICRO = [("homo", None, 128, 13, 5, 4, 0.5), ("hetero", None, 128, 13, 5, 4, 0.9), ("pagg", None, 32, 13, 5, 4, 0.1),
         ("hetero", None, 288, 13, 5, 4, 0.5), ("homo", "sum", 96, 13, 5, 4, 0.5), ("homo", "gru", 100, 13, 5, 4, 0.5)]


@pytest.mark.parametrize("case", MICRO, ids=dp.case_id)
@pytest.mark.parametrize("math", ["f16x2", "bf16x3"])
def test_micro_batches_keep_whole_batch_counters(case, math, monkeypatch):
    """13 masked nodes walked 4 at a time (pick_batch_groups, as tests/test_gpu_batching.py sets it): the forward's bits, the
    bits of the backward's re-run and the classifier's are those of the one batch"""
    from pathnet_amd import modules
    variant, cell, H, S, W, L, p = case
    monkeypatch.setattr(modules, "pick_batch_groups", lambda *a, **k: 4)
    m = _module(variant, cell, H, L, p, math)
    sel, ids, codes = dp.paths(S, W, L, seed=4)
    ms, mc = _masks(_seed_of("torch"), p, L, S, W, H)
    assert torch.equal(_forward_bits(m, case, torch.zeros(N, H, device="cuda"), sel, ids, codes, "torch"), ms != 0)
    node = po.plan(variant, ids, codes, S, W, L)[0]
    assert torch.equal(dp.backward_bits(_backward_x_grad(m, case, sel, ids, codes, "torch"), node), ms != 0)
    if cell not in dp.REDUCING:
        args = _index_args(sel, ids, codes, W, L)

        def run(X):
            torch.manual_seed(TORCH_SEED)
            return m(X, *args)
        bits, xg = _classifier_read(m, case, run)
        assert torch.equal(bits, mc != 0)
        assert torch.equal(dp.joint_bits(xg, sel, node, S, W, C, variant)[0], mc[:, :H] != 0)


@pytest.mark.parametrize("variant,cell,H,p", [("homo", None, 128, 0.5), ("hetero", None, 96, 0.9), ("pagg", None, 32, 0.1),
                                              ("hetero", "gru", 288, 0.5), ("hetero", "mean", 128, 0.5)])
def test_group_slice_keeps_whole_batch_counters(variant, cell, H, p):
    """slices [0, 5) and [5, 13) of a batch of 13: together every bit of the whole batch's masks"""
    S, W, L = 13, 5, 4
    case = (variant, cell, H, S, W, L, p)
    m = _module(variant, cell, H, L, p)
    sel, ids, codes = dp.paths(S, W, L, seed=5)
    ms, mc = _masks(2 ** 62 - 1, p, L, S, W, H)
    node = po.plan(variant, ids, codes, S, W, L)[0]
    bits = torch.zeros(L, S * W, H, dtype=torch.bool)
    bwd = torch.zeros_like(bits)
    cls_rows = []
    for begin, count in ((0, 5), (5, 8)):
        _forward_bits(m, case, torch.zeros(N, H, device="cuda"), sel, ids, codes, "max", begin, count, bits)
        bwd |= dp.backward_bits(_backward_x_grad(m, case, sel, ids, codes, "max", group_slice=(begin, count)), node)
        if cell not in dp.REDUCING:
            _load(m, dp.params(variant, cell, H, L, C, dp.amp_every_step(p, L), cell_bias=1.0))
            m.zero_grad(set_to_none=True)
            enc = _encode(m, torch.zeros(N, H, device="cuda"), sel, ids, codes, W, L, "max", group_slice=(begin, count))
            assert float(enc.embedding.detach().min()) > 0.0
            (enc.logits * torch.eye(count, C, device="cuda")).sum().backward()
            cls_rows.append(m.fc2.weight.grad[:count].cpu() != 0)
    assert torch.equal(bits, ms != 0)
    assert torch.equal(bwd, ms != 0)            # (a slice's backward shows its own slots only: the two together, all)
    if cls_rows:
        assert torch.equal(torch.cat(cls_rows), mc != 0)


@pytest.mark.parametrize("variant,cell,H,p", [("homo", None, 128, 0.9), ("homo", "gru", 32, 0.5), ("pagg", None, 96, 0.1)])
def test_batch_position_keeps_whole_batch_counters(variant, cell, H, p):
    """a data-parallel rank's call: the index arrays hold its own rows only, the counters are positions in the whole batch"""
    S, W, L = 13, 5, 4
    m = _module(variant, cell, H, L, p)
    sel, ids, codes = dp.paths(S, W, L, seed=6)
    seed = dr.module_seed(TORCH_SEED)
    ms, mc = _masks(seed, p, L, S, W, H)
    bits = torch.zeros(L, S * W, H, dtype=torch.bool)
    cls_rows = []
    for begin, count in ((0, 5), (5, 8)):
        rows = slice(begin, begin + count)
        neis = torch.as_tensor(ids[rows].reshape(count, W * L).astype(np.int64))
        lt = torch.as_tensor(codes[rows].astype(np.int64))
        slot = dp.slots(variant, S, W, begin, count)
        for t in range(L):
            _load(m, dp.params(variant, cell, H, L, C, dp.amp_one_step(p, L, t)))
            res = m._run(torch.zeros(N, H, device="cuda"), neis, W, L, sel[rows].astype(np.int64), lt,
                         batch_position=(S, begin), seed=seed, _encode=True)
            dp.put_forward_bits(bits, t, res[3], slot)
        _load(m, dp.params(variant, cell, H, L, C, dp.amp_every_step(p, L), cell_bias=1.0))
        m.zero_grad(set_to_none=True)
        res = m._run(torch.zeros(N, H, device="cuda"), neis, W, L, sel[rows].astype(np.int64), lt,
                     batch_position=(S, begin), seed=seed, _encode=True)
        assert float(res[1].detach().min()) > 0.0
        (res[0] * torch.eye(count, C, device="cuda")).sum().backward()
        cls_rows.append(m.fc2.weight.grad[:count].cpu() != 0)
    assert torch.equal(bits, ms != 0)
    assert torch.equal(torch.cat(cls_rows), mc != 0)


@pytest.mark.parametrize("variant,H,p", [("homo", 128, 0.5), ("hetero", 32, 0.9)])
def test_step_state_seeds(variant, H, p):
    """a StepState advanced three times: the seed the kernels read from device memory is splitmix64's, step by step"""
    import pathnet_amd
    S, W, L = 11, 3, 4
    case = (variant, None, H, S, W, L, p)
    m = _module(variant, None, H, L, p)
    st = pathnet_amd.StepState("cuda", seed=1234, first_epoch=0)
    m.step_state = st
    want = {"epoch": -1, "seed": 1234, "adam_step": 0}
    sel, ids, codes = dp.paths(S, W, L, seed=7)
    node = po.plan(variant, ids, codes, S, W, L)[0]
    args = _index_args(sel, ids, codes, W, L)
    for _ in range(3):
        st.advance()
        want = splitmix_advance(want)
        assert st.values() == want
        ms, mc = dr.module_masks(want["seed"], p, L, S, W, H)
        assert torch.equal(_forward_bits(m, case, torch.zeros(N, H, device="cuda"), sel, ids, codes, "zero"), ms != 0)
        assert torch.equal(dp.backward_bits(_backward_x_grad(m, case, sel, ids, codes, "zero"), node), ms != 0)
        bits, _ = _classifier_read(m, case, lambda X: m(X, *args))
        assert torch.equal(bits, mc != 0)


@pytest.mark.parametrize("variant,S,W,L,p,bg", [("homo", 13, 5, 4, 0.5, 0), ("hetero", 11, 3, 4, 0.9, 0), ("pagg", 13, 5, 4, 0.1, 4)])
def test_fused_step_masks(variant, S, W, L, p, bg, monkeypatch):
    """forward_loss(fused=True): the logits are the oracle's under the reference masks, and the step's own backward shows
    the classifier's ego half on the masked nodes' rows and sequence bit AND pooled bit on every path step's row"""
    from pathnet_amd import modules
    H = 128
    monkeypatch.setattr(modules, "pick_batch_groups", lambda *a, **k: bg)
    m = _module(variant, None, H, L, p)
    sel, ids, codes = dp.paths(S, W, L, seed=8)
    sd = dp.params(variant, None, H, L, C, dp.amp_every_step(p, L), cell_bias=1.0)
    sd["fc2.weight"] = ((torch.arange(C) + 1.0) / C)[:, None].expand(C, 2 * H).contiguous()
    _load(m, sd)
    seed = dr.module_seed(TORCH_SEED)
    ms, mc = _masks(seed, p, L, S, W, H)
    X = torch.zeros(N, H, device="cuda", requires_grad=True)
    target = torch.zeros(S, dtype=torch.int64)      # class 0 carries the smallest weights: d loss / d layer1 > 0 everywhere
    torch.manual_seed(TORCH_SEED)
    loss, out = m.forward_loss(X, *_index_args(sel, ids, codes, W, L)[:5], target, fused=True)
    loss.backward()
    r = dp.oracle_run(variant, None, sd, torch.zeros(N, H), sel, ids, codes, W, L, ms, mc)
    assert (out.cpu() - r["logits"]).abs().max().item() < 1e-5 * max(1.0, r["logits"].abs().max().item())
    xg = X.grad.cpu()
    node = po.plan(variant, ids, codes, S, W, L)[0]
    group = dp.group_of(variant, S, W)
    assert torch.equal(xg[torch.as_tensor(sel)] != 0, mc[:, :H] != 0)
    assert torch.equal(dp.backward_bits(xg, node), (ms != 0) & (mc[:, H:] != 0)[torch.as_tensor(group)][None])


# ---- values at ordinary weights: the cases held to the bf16 x 3 kernels elsewhere, held to the oracle -----------------------
def _hold(out, g, o32, g32, o64, g64, zero_ok):
    """The suite's contract against the fp32 oracle: logits within 1e-5, gradients by tests/gradcheck.py.  Where the fp32
    oracle itself is farther than that from fp64 (o64 given: p = 0.9 scales x by 10), the rule of tests/test_gpu_seqh.py's
    _against_fp64: 8 x stock fp32 torch's distance from fp64, or a floor of 2e-6."""
    assert not torch.isnan(out).any()
    e_t = (o32.double() - o64).abs().max().item() if o64 is not None else 0.0
    e32 = (out - o32).abs().max().item()
    print("logits: |hip - fp32 oracle| %.3g, |fp32 oracle - fp64| %.3g" % (e32, e_t))
    if e_t <= 1e-5:
        assert e32 < 1e-5, e32
    else:
        e_hip = (out.double() - o64).abs().max().item()
        assert e_hip <= max(8.0 * e_t, 2e-6 * max(1.0, o64.abs().max().item())), ("logits", e_hip, e_t)
    rows64 = grad_report(g32, g64, GRAD_REL, NOISE)[0] if g64 is not None else {}
    if all(e <= t for e, t, _ in rows64.values()):
        assert_grads_close(g, g32, zero_ok=zero_ok)
        return
    for k in g:
        scale = max(g64[k].abs().max().item(), 1e-300)
        e_hip = (g[k].double() - g64[k]).abs().max().item()
        e_k = (g32[k].double() - g64[k]).abs().max().item()
        print("%s: |hip - fp64| %.3g, |fp32 oracle - fp64| %.3g, scale %.3g" % (k, e_hip, e_k, scale))
        assert e_hip <= max(8.0 * e_k, 2e-6 * scale), (k, e_hip, e_k, scale)


def _oracle_grads(variant, cell, m, X, ids, codes, sel, G, W, L, masks, dtype):
    params = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in m.state_dict().items()}
    want = po.forward(variant, params, X, ids, codes, sel, W, L, drop_seq=masks[0], drop_cls=masks[1], dtype=dtype, cell=cell)
    want.backward(G.to(dtype))
    return want.detach(), {k: params[k].grad if params[k].grad is not None else torch.zeros_like(params[k])
                           for k, _ in m.named_parameters()}


def _builtin_cases():
    from test_gpu_bwdh_edges import BUILTIN_CASES
    return BUILTIN_CASES


@pytest.mark.parametrize("variant,cell,H,S,W,L", _builtin_cases())
def test_bptt_edges_with_built_in_dropout_match_the_oracle(variant, cell, H, S, W, L):
    import test_gpu_bwdh_edges as e
    m = e._module(variant, cell, H, L, 0.7)
    X, sel, ids, codes, _, _, G = e._inputs(S, W, L, H, seed=12)
    out, g = e._hip(m, X, sel, ids, codes, G, W, L)             # (torch.manual_seed(7) inside)
    masks = _masks(dr.module_seed(7), 0.7, L, S, W, H)
    o32, g32 = _oracle_grads(variant, cell, m, X, ids, codes, sel, G, W, L, masks, torch.float32)
    _hold(out, g, o32, g32, None, None, e._zero_ok(variant))


def _seqh_dropout_rows():
    import test_gpu_seqh as s
    mark = [k for k in s.test_f16_kernels_match_the_bf16_kernels.pytestmark if k.name == "parametrize"][0]
    return [row for row in mark.args[1] if row[6] > 0.0]


@pytest.mark.parametrize("math", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("variant,H,S,W,L,cell,drop", _seqh_dropout_rows())
def test_recurrent_kernels_with_built_in_dropout_match_the_oracle(variant, H, S, W, L, cell, drop, math):
    import test_gpu_seqh as s
    from gradcheck import ZERO_OK_HETERO
    case = s._case(variant, H, S, W, L, cell, drop)
    m, X, ids, codes, sel, G = case
    out, g = s._run(case, math)                                 # (torch.manual_seed(7) inside)
    masks = _masks(dr.module_seed(7), drop, L, S, W, H)
    a = (variant, cell, m, X.cpu(), ids.cpu().numpy(), codes.cpu().numpy(), sel.cpu().numpy(), G.cpu(), W, L, masks)
    o32, g32 = _oracle_grads(*a, torch.float32)
    o64, g64 = _oracle_grads(*a, torch.float64) if drop >= 0.9 else (None, None)
    _hold(out.cpu(), {k: v.cpu() for k, v in g.items()}, o32, g32, o64, g64, ZERO_OK_HETERO if variant == "hetero" else ())


@pytest.mark.parametrize("variant,cell,H,S,W,L,p", [("homo", None, 128, 13, 5, 4, 0.7), ("hetero", None, 128, 11, 3, 4, 0.5)])
def test_fused_step_with_built_in_dropout_matches_the_oracle(variant, cell, H, S, W, L, p):
    """forward_loss(fused=True): loss, logits and every gradient against the oracle + cross_entropy_ref under the
    reconstructed masks"""
    import test_gpu_bwdh_edges as e
    m = e._module(variant, cell, H, L, p)
    X, sel, ids, codes, _, _, _ = e._inputs(S, W, L, H, seed=15)
    y = torch.as_tensor(np.random.default_rng(15).integers(0, e.C, S))
    node_mask = np.zeros(e.N, bool)
    node_mask[sel] = True
    torch.manual_seed(7)
    m.zero_grad(set_to_none=True)
    loss, out = m.forward_loss(X.cuda(), torch.as_tensor(ids.reshape(S, W * L).astype(np.int64)), W, L, node_mask,
                               torch.as_tensor(codes.astype(np.int64)), y, fused=True)
    loss.backward()
    g = {k: v.grad.detach().cpu() for k, v in m.named_parameters()}
    masks = _masks(dr.module_seed(7), p, L, S, W, H)
    params = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    want = po.forward(variant, params, X, ids, codes, sel, W, L, drop_seq=masks[0], drop_cls=masks[1], cell=cell)
    l64, g64, _, _ = cross_entropy_ref(want, y)
    want.backward(g64.float())
    ref = {k: params[k].grad if params[k].grad is not None else torch.zeros_like(params[k]) for k, _ in m.named_parameters()}
    assert (out.cpu() - want.detach()).abs().max().item() < 1e-5
    assert abs(loss.item() - l64) < 1e-5
    assert_grads_close(g, ref, zero_ok=e._zero_ok(variant))
