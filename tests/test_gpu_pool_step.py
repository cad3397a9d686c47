"""The training step's pooling launch (pn_pagg_train_step, default mode: attention + pooling + classifier, softmax cross
entropy and the pooling backward of a node in one workgroup) against the fp64 oracle, at the edges of its dispatch rule
(launch_pool_step in pn_pool.hip; Hk = the hidden size padded to a multiple of 32):

    PN_POOL_STEP = 1, W <= 40, 32 <= Hk <= 128, pool_step2_lds_bytes(10, Hk, C) <= 64 KiB   -> pool_step2_kernel<10, 2>
    otherwise, Hk <= 256                                                                     -> pool_step_kernel<4>
    otherwise                                                                                -> pool_step_kernel<16>

PN_POOL_STEP = 2 skips the register kernel, 0 runs the three launches (pool_fwd_kernel, cross_entropy_kernel,
pool_bwd_wg_kernel), and the deterministic mode always runs the three launches.  Every case runs in all four settings and
in the eval forward (pool_fwd_kernel), each held against ONE fp64 evaluation of oracle/pagg_oracle.py with the same
dropout masks, to the suite's bounds: logits and loss within 1e-5 * max(1, |ref|), every parameter gradient and X's by
tests/gradcheck.py.  (test_gpu_fused_step.py compares these kernels with one another.)"""
import numpy as np
import pytest
import torch
from gradcheck import ZERO_OK_HETERO, assert_grads_close, named_grads

from oracle import pagg_oracle as po

pytestmark = pytest.mark.gpu

N, F, L = 900, 40, 4
TOL = 1e-5
# (name, PN_POOL_STEP, deterministic)
MODES = (("registers", 1, False), ("pool_step", 2, False), ("three_launches", 0, False), ("deterministic", 1, True))


class Case:
    """A module, a batch of S masked nodes with W paths each, targets 0 and C - 1 among them, explicit dropout masks."""

    def __init__(self, variant, S, W, H, C, cell=None, seed=0, split_ego=False, fc2_scale=None, loss_weight=1.0, micro=0,
                 min_logit=None):
        import pathnet_amd
        torch.manual_seed(seed)
        rng = np.random.default_rng(seed)
        cls = {"homo": pathnet_amd.PathNet_homo, "hetero": pathnet_amd.PathNet, "pagg": pathnet_amd.PAGG}[variant]
        self.m = cls(F, H, C, L, dropout=0.5, **({} if variant == "pagg" else {"cell": cell})).cuda()
        if fc2_scale is not None:
            with torch.no_grad():
                self.m.fc2.weight.mul_(fc2_scale)
        self.variant, self.S, self.W, self.H, self.C, self.cell = variant, S, W, H, C, cell
        self.X = torch.rand(N, F)
        sel = np.sort(rng.choice(N, S, replace=False))
        ids = rng.integers(0, N, (S, W, L))
        ids[:, :, 0] = sel[:, None]
        if split_ego:
            # paths of a node that start at another node (HOMO: the member's ego row is then not the node's -- the kernels'
            # per-member branch): member 0 of every third node, the last member of every fifth, wave 1's slot 9 of every
            # seventh; the other nodes keep one ego row
            ids[::3, 0, 0] = (sel[::3] + 1) % N
            ids[::5, W - 1, 0] = (sel[::5] + 2) % N
            ids[::7, 37, 0] = (sel[::7] + 3) % N
        # distance codes as the sampler gives them: 0 at the start, at most t at step t
        codes = np.minimum(rng.integers(0, L, (S, W, L)), np.arange(L)[None, None, :])
        y = rng.integers(0, C, S)
        y[0], y[-1] = 0, C - 1
        self.ids, self.codes, self.sel, self.y = ids, codes, sel, torch.as_tensor(y)
        self.mask_seq = (torch.rand(L, S * W, H) < 0.5).float() / 0.5
        self.mask_cls = (torch.rand(S, 2 * H) < 0.5).float() / 0.5
        self.loss_weight, self.micro = loss_weight, micro
        self.min_logit = min_logit      # the fp64 oracle's largest |logit| must exceed it (run_all asserts)
        self.zero_ok = ZERO_OK_HETERO if variant == "hetero" else ()
        self.dev = (torch.as_tensor(ids, dtype=torch.int32).cuda(), torch.as_tensor(codes, dtype=torch.uint8).cuda(),
                    torch.as_tensor(sel, dtype=torch.int32).cuda(), self.y.cuda())

    def budget(self, det):
        """micro > 0: a workspace budget for micro-batches of `micro` masked nodes"""
        if not self.micro:
            return None
        from pathnet_amd import modules as M
        Hk = -(-self.H // 32) * 32
        kw = dict(cell=self.m._cell_kind, deterministic=det)
        b = M.workspace_bytes(self.variant, N, F, Hk, self.C, self.S, self.W, L, batch_groups=self.micro, **kw)
        assert M.pick_batch_groups(self.variant, N, F, Hk, self.C, self.S, self.W, L, b, **kw) == self.micro
        return b

    def oracle(self, train):
        """(loss, logits, {name: gradient}) in fp64: the training step's loss_weight * mean cross entropy; eval: logits"""
        params = {k: v.detach().cpu().double().requires_grad_(train) for k, v in self.m.state_dict().items()}
        X = self.X.double().requires_grad_(train)
        kw = dict(drop_seq=self.mask_seq, drop_cls=self.mask_cls) if train else {}
        with torch.set_grad_enabled(train):
            out = po.forward(self.variant, params, X, self.ids, self.codes, self.sel, self.W, L, dtype=torch.float64,
                             cell=self.cell, **kw)
        if not train:
            return None, out, None
        loss = self.loss_weight * torch.nn.functional.cross_entropy(out, self.y)
        loss.backward()
        grads = {k: params[k].grad for k, _ in self.m.named_parameters()}
        grads["X"] = X.grad
        return loss.item(), out.detach(), grads

    def step(self, knob, det):
        """the fused training step (m.forward_loss(..., fused=True)) with PN_POOL_STEP = knob"""
        from pathnet_amd import _lib
        m = self.m
        ids, codes, sel, y = self.dev
        m.train()
        m.deterministic = det
        m.workspace_budget = self.budget(det)
        m._mask_seq, m._mask_cls = self.mask_seq.cuda(), self.mask_cls.cuda()
        m.zero_grad(set_to_none=True)
        X = self.X.cuda().requires_grad_(True)
        gs = None if self.loss_weight == 1.0 else self.loss_weight / self.S
        old = _lib.set_knob("PN_POOL_STEP", knob)
        try:
            loss, out = m.forward_loss(X, ids, self.W, L, sel, codes, y, grad_scale=gs, fused=True)
            loss.backward()
            torch.cuda.synchronize()
        finally:
            _lib.set_knob("PN_POOL_STEP", old)
        return loss.item(), out.detach().cpu().double(), named_grads(m, {"X": X.grad})

    def eval_forward(self):
        ids, codes, sel, _ = self.dev
        self.m.eval()
        with torch.no_grad():
            out = self.m(self.X.cuda(), ids, self.W, L, sel, codes, None)
        torch.cuda.synchronize()
        return out.cpu().double()


def _check_logits(tag, out, ref):
    err = (out - ref).abs().max().item()
    assert err <= TOL * max(1.0, ref.abs().max().item()), "%s: logits off by %.3g (|ref| %.3g)" % (tag, err, ref.abs().max())


def run_all(case, modes=MODES):
    """every pooling path of the case against the one fp64 reference; the eval forward against the eval reference"""
    rl, ro, rg = case.oracle(train=True)
    if case.min_logit is not None:
        assert ro.abs().max().item() > case.min_logit, "largest |logit| %.3g" % ro.abs().max().item()
    for name, knob, det in modes:
        tag = "%s (PN_POOL_STEP=%d, deterministic=%s)" % (name, knob, det)
        loss, out, grads = case.step(knob, det)
        _check_logits(tag, out, ro)
        assert abs(loss - rl) <= TOL * max(1.0, abs(rl)), "%s: loss %.9g, oracle %.9g" % (tag, loss, rl)
        try:
            assert_grads_close(grads, rg, zero_ok=case.zero_ok, tag=tag)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (tag, e)) from None
    _check_logits("eval forward", case.eval_forward(), case.oracle(train=False)[1])


# kernel under PN_POOL_STEP = 1 (Hk = the padded hidden size):  step2 = pool_step2_kernel<10, 2>, step<4> / step<16> =
# pool_step_kernel<4> / <16>
CASES = {
    # headline shape, all ten member slots of a wave (S ~ 300, Cora-like): step2
    "homo_W40_H128_C7": dict(variant="homo", S=300, W=40, H=128, C=7),
    # Cornell flagship, softmax over 40 lanes: step2
    "hetero_W40_H128_C5": dict(variant="hetero", S=200, W=40, H=128, C=5),
    # no attention: step2, column slot 1 fully masked
    "pagg_W40_H64_C5": dict(variant="pagg", S=150, W=40, H=64, C=5),
    # 37 = 4 * 9 + 1 members: wave 0 holds ten, the others nine; H = 96 masks half of column slot 1: step2
    "homo_W37_H96_C3": dict(variant="homo", S=120, W=37, H=96, C=3),
    "hetero_W37_H96_C3": dict(variant="hetero", S=120, W=37, H=96, C=3),
    # a single member (the softmax over one path is 1); H = 32: step2
    "hetero_W1_H32_C2": dict(variant="hetero", S=60, W=1, H=32, C=2),
    # small W, not a multiple of 4: step2
    "pagg_W5_H32_C4": dict(variant="pagg", S=80, W=5, H=32, C=4),
    "homo_W5_H32_C4": dict(variant="homo", S=80, W=5, H=32, C=4),
    # just past the register kernel in W: step<4>
    "homo_W41_H128_C7": dict(variant="homo", S=100, W=41, H=128, C=7),
    # just past the register kernel in H: step<4>
    "hetero_W40_H160_C5": dict(variant="hetero", S=100, W=40, H=160, C=5),
    # H > 256, generic recurrence: step<16>
    "homo_gru_W12_H288_C5": dict(variant="homo", S=60, W=12, H=288, C=5, cell="gru"),
    # H = 100 zero-padded to Hk = 128, order-agnostic encoder: step2
    "homo_mean_W40_H100_C5": dict(variant="homo", S=100, W=40, H=100, C=5, cell="mean"),
    # the cross entropy's class loops past one wave of lanes: step2
    "hetero_W40_H128_C65": dict(variant="hetero", S=60, W=40, H=128, C=65),
    "hetero_W40_H128_C257": dict(variant="hetero", S=60, W=40, H=128, C=257),
    # members whose ego row is not the node's (the per-member ego atomics): step2
    "homo_split_ego_W40_H128_C5": dict(variant="homo", S=105, W=40, H=128, C=5, split_ego=True),
    # saturated softmax: fc2 x 50, some logits' gradients ~0 and others ~ -1 / S: step2
    "homo_saturated_W40_H128_C7": dict(variant="homo", S=100, W=40, H=128, C=7, fc2_scale=50.0),
    # logits past 1e3 (fc2 x 1000: the oracle's largest is 1.27e3): the softmax must not lose bits with their size: step2
    "homo_large_logits_W40_H128_C7": dict(variant="homo", S=100, W=40, H=128, C=7, fc2_scale=1000.0, min_logit=1e3),
    # three micro-batches of 34, 34 and 32 nodes, the loss added over them: step2
    "homo_micro_W40_H128_C7": dict(variant="homo", S=100, W=40, H=128, C=7, micro=34),
    "hetero_micro_W40_H128_C7": dict(variant="hetero", S=100, W=40, H=128, C=7, micro=34),
    # grad_scale = 2.5 / S: the loss is 2.5 * the mean: step2
    "homo_grad_scale_W40_H128_C7": dict(variant="homo", S=100, W=40, H=128, C=7, loss_weight=2.5),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_pool_step_matches_the_fp64_oracle(name):
    run_all(Case(**CASES[name]))


def test_largest_walk_count_runs_and_the_next_is_refused():
    """make_dims budgets the pooling kernels' LDS (pool_lds_bytes, pn_pool.hip: 64 W + 48 H bytes) at 64 KiB: W = 928 at H = 128 is the largest W it
    accepts (step<4>, 64 KiB of LDS, in every mode) and matches the oracle; W = 929 is refused with PN_ERR_ARG."""
    from pathnet_amd import _lib
    run_all(Case("homo", S=3, W=928, H=128, C=5))
    case = Case("homo", S=3, W=929, H=128, C=5)
    with pytest.raises(_lib.PnError) as e:
        case.step(1, False)
    assert e.value.code == _lib.PN_ERR_ARG


def test_classes_past_the_register_kernels_lds():
    """pool_step2_kernel keeps the logits and their gradient in LDS: 6 144 + 8 C bytes at H = 128, past 64 KiB for
    C > 7 424.  C = 8 000 goes to pool_step_kernel<4> (LDS independent of C) and matches the oracle, targets 0 and C - 1."""
    run_all(Case("homo", S=6, W=40, H=128, C=8000))
