"""The touched-row ("compact") distance bank against the fp64 oracle (pn_pagg.hip: run_compact_rows, the compact branches of
run_tables and run_bank_bwd; the flag / scan kernels: pn_plan.hip).  make_dims switches to it when 2 * S * W * L < N * L -- every ordinary mini-batch of a large
graph -- and PN_COMPACT=1 forces it.  Its row counts exist in device memory only (seg[code], seg[L]) while its launches are
sized by the host-side bound mmax = min(N, ZR), so the cases are built by construction at the edges where such kernels go
wrong: a code no path touches, per-code segments of 63 / 64 / 65 / 127 / 128 / 129 rows (the 64 x 64 GEMM tile, the
128 x 128 rgrad tile), every (node, code) row touched, a single touched row, nodes 0 and N - 1 at every code, N * L not a
multiple of 16 (scan_count_kernel's scalar tail), a second call that touches fewer rows than the first, a spike row among
the touched ones (launch_range_rows counts seg[L] rows).

Every case runs the eval forward, encode(path_state=True), a group_slice, forward + backward (default and deterministic:
launch_gemm_det over GEMM_IND_K), the fused step under PN_POOL_STEP 0 / 1 / 2 and, where it says so, micro-batches, each
held against ONE fp64 evaluation of oracle/pagg_oracle.py with the same dropout masks, to the suite's bounds: logits, loss
and the encoder's outputs within 1e-5 * max(1, |ref|), every gradient and X's by tests/gradcheck.py.  Each case fixes the
node-level GEMM route of the compact backward with PN_NODE_RGRAD (0: the atomic GEMM over GEMM_IND_K, 1: rgrad_kernel
from 2 048 rows, 2: rgrad_kernel with LIST -- and GATE for the homo class -- at any size)."""
import numpy as np
import pytest
import torch
from gradcheck import ZERO_OK_HETERO, assert_grads_close, named_grads

from oracle import pagg_oracle as po
from test_gpu_batching import no_relu_ties

pytestmark = pytest.mark.gpu

F = 16
TOL = 1e-5


def plan_to_paths(variant, node, code, S, W, L):
    """ids / codes [S, W, L] whose index plan (oracle/pagg_oracle.py: plan) is node / code [P, L]: the hetero class reads
    node (q, t) from ids[r % P, L - 1 - r // P], r = q * L + t, and the code from codes[q, t]"""
    P = S * W
    if variant == "hetero":
        r = np.arange(P * L)
        ids = np.empty((P, L), np.int64)
        ids[r % P, L - 1 - r // P] = node.reshape(-1)
    else:
        ids = node.copy()
    return ids.reshape(S, W, L), code.reshape(S, W, L).copy()


def touched_rows(variant, ids, codes, S, W, L):
    """{code: sorted distinct nodes} the call's paths touch (what run_compact_rows must find)"""
    node, code = po.plan(variant, ids, codes, S, W, L)[:2]
    return {c: np.unique(node[code == c]) for c in range(L)}


def structured_plan(rng, P, L, sets):
    """node / code [P, L] that touch exactly the (node, code) rows sets[c] (empty: a code no path uses); the codes of the
    steps are spread evenly over the codes in use, every row of a set at least once"""
    used = [c for c in range(L) if len(sets[c])]
    code = np.asarray(used)[rng.permutation(np.arange(P * L) % len(used))].reshape(P, L)
    node = np.empty(P * L, np.int64)
    for c in used:
        pos = np.flatnonzero(code.reshape(-1) == c)
        assert len(pos) >= len(sets[c]), "too few steps for code %d" % c
        node[pos] = rng.permutation(np.concatenate([sets[c], rng.choice(sets[c], len(pos) - len(sets[c]))]))
    return node.reshape(P, L), code


def row_sets(kind, rng, N, L, sizes=None):
    """the touched rows per code of a structure: `sizes` nodes at code c (nodes 0 and N - 1 among them when there are two
    or more), all N nodes at every code, or one (node, code) row"""
    if kind == "sizes":
        out = []
        for n in sizes:
            mid = rng.choice(np.arange(1, N - 1), max(n - 2, 0), replace=False)
            out.append(np.sort(np.concatenate([[0, N - 1], mid]))[:n] if n >= 2 else np.arange(n) + N // 2)
        return out
    if kind == "all":
        return [np.arange(N)] * L
    if kind == "one":
        return [np.array([N - 1]) if c == L - 2 else np.array([], np.int64) for c in range(L)]
    if kind == "last":                  # `sizes` rows per code, node N - 1 at the last code only: the last compact row
        out = [rng.choice(N - 1, n, replace=False) for n in sizes]
        out[-1] = np.concatenate([out[-1][:-1], [N - 1]])
        return [np.sort(r) for r in out]
    if kind == "ends":                  # random rows, nodes 0 and N - 1 at every code
        return [np.unique(np.concatenate([[0, N - 1], rng.choice(N, N // 3, replace=False)])) for _ in range(L)]
    raise ValueError(kind)


class Case:
    """A module, a batch of S masked nodes with W paths each, targets 0 and C - 1 among them, explicit dropout masks;
    paths: "random" (codes as the sampler gives them: at most t at step t) or a structure of row_sets"""

    def __init__(self, variant, N, S, W, L=4, H=128, C=5, cell=None, math=None, paths="random", sizes=None, seed=0,
                 micro=0, rgrad=1, auto=False):
        import pathnet_amd
        torch.manual_seed(seed)
        rng = np.random.default_rng(seed)
        cls = {"homo": pathnet_amd.PathNet_homo, "hetero": pathnet_amd.PathNet, "pagg": pathnet_amd.PAGG}[variant]
        self.m = cls(F, H, C, L, dropout=0.5, **({} if variant == "pagg" else {"cell": cell})).cuda()
        if math is not None:
            self.m.seq_math = math
        if auto and variant == "homo":
            no_relu_ties(self.m)
        self.variant, self.N, self.S, self.W, self.L, self.H, self.C, self.cell = variant, N, S, W, L, H, C, cell
        self.micro, self.rgrad, self.auto = micro, rgrad, auto
        self.X = torch.rand(N, F)
        self.sel = np.sort(rng.choice(N - 1 if paths == "last" else N, S, replace=False))
        P = S * W
        if paths == "random":
            node = rng.integers(0, N, (P, L))
            code = np.minimum(rng.integers(0, L, (P, L)), np.arange(L)[None, :])
            self.sets = None
        else:
            self.sets = row_sets(paths, rng, N, L, sizes)
            node, code = structured_plan(rng, P, L, self.sets)
        self.ids, self.codes = plan_to_paths(variant, node, code, S, W, L)
        if self.sets is not None:       # the construction touches exactly the rows it was asked for
            got = touched_rows(variant, self.ids, self.codes, S, W, L)
            for c in range(L):
                assert np.array_equal(got[c], np.unique(self.sets[c])), c
        y = rng.integers(0, C, S)
        y[0], y[-1] = 0, C - 1
        self.y = torch.as_tensor(y)
        self.mask_seq = (torch.rand(L, P, H) < 0.5).float() / 0.5
        self.mask_cls = (torch.rand(S, 2 * H) < 0.5).float() / 0.5
        self.zero_ok = ZERO_OK_HETERO if variant == "hetero" else ()
        self.dev = (torch.as_tensor(self.ids, dtype=torch.int32).cuda(), torch.as_tensor(self.codes, dtype=torch.uint8).cuda(),
                    torch.as_tensor(self.sel, dtype=torch.int32).cuda(), self.y.cuda())

    def ran_compact(self):
        from pathnet_amd import modules as M
        return M.shape_info(self.m._last_shape[0])[0]

    def budget(self, det):
        from pathnet_amd import modules as M
        Hk = -(-self.H // 32) * 32
        kw = dict(cell=self.m._cell_kind, deterministic=det)
        b = M.workspace_bytes(self.variant, self.N, F, Hk, self.C, self.S, self.W, self.L, batch_groups=self.micro, **kw)
        assert M.pick_batch_groups(self.variant, self.N, F, Hk, self.C, self.S, self.W, self.L, b, **kw) == self.micro
        return b

    def oracle(self, train):
        """train: (loss, logits, {name: gradient}) of the mean cross entropy with the case's masks; eval: (logits,
        embedding, path weights, path states).  fp64."""
        params = {k: v.detach().cpu().double().requires_grad_(train) for k, v in self.m.state_dict().items()}
        X = self.X.double().requires_grad_(train)
        kw = dict(drop_seq=self.mask_seq, drop_cls=self.mask_cls) if train else {}
        S, W = self.S, self.W
        with torch.set_grad_enabled(train):
            out, it = po.forward(self.variant, params, X, self.ids, self.codes, self.sel, W, self.L, dtype=torch.float64,
                                 cell=self.cell, return_intermediates=True, **kw)
        if not train:
            emb = torch.cat([it["Xh"][torch.as_tensor(self.sel, dtype=torch.long)], it["pooled"]], dim=1)
            att = it["att"]
            pw = (att.view(S, W) if self.variant == "hetero" else 1.0 + att.view(S, W) if self.variant == "homo"
                  else torch.ones(S, W, dtype=torch.float64))
            s, j = np.meshgrid(np.arange(S), np.arange(W), indexing="ij")
            q = j * S + s if self.variant == "hetero" else s * W + j
            ps = it["h"][torch.as_tensor(q.reshape(-1))].view(S, W, -1)
            return out, emb, pw, ps
        loss = torch.nn.functional.cross_entropy(out, self.y)
        loss.backward()
        # (a distance layer no path of the case uses has no reference gradient: it must come back as zeros)
        grads = {k: params[k].grad if params[k].grad is not None else torch.zeros_like(params[k])
                 for k, _ in self.m.named_parameters()}
        grads["X"] = X.grad
        return loss.item(), out.detach(), grads

    def step(self, det, fused, micro=False):
        """forward_loss: fused (pn_pagg_train_step) or forward + cross entropy + backward; micro: the case's micro-batches"""
        m = self.m
        ids, codes, sel, y = self.dev
        m.train()
        m.deterministic = det
        m.workspace_budget = self.budget(det) if micro else None
        m._mask_seq, m._mask_cls = self.mask_seq.cuda(), self.mask_cls.cuda()
        m.zero_grad(set_to_none=True)
        X = self.X.cuda().requires_grad_(True)
        loss, out = m.forward_loss(X, ids, self.W, self.L, sel, codes, y, fused=fused)
        loss.backward()
        torch.cuda.synchronize()
        m.workspace_budget = None
        return loss.item(), out.detach().cpu().double(), named_grads(m, {"X": X.grad})

    def eval_call(self, encode=False, group_slice=None):
        ids, codes, sel, _ = self.dev
        self.m.eval()
        with torch.no_grad():
            if encode:
                r = self.m.encode(self.X.cuda(), ids, self.W, self.L, sel, codes, None, path_state=True)
                r = tuple(t.cpu().double() for t in r)
            else:
                r = self.m(self.X.cuda(), ids, self.W, self.L, sel, codes, None, group_slice=group_slice).cpu().double()
        torch.cuda.synchronize()
        return r


def _close(tag, got, ref):
    err = (got - ref).abs().max().item()
    assert err <= TOL * max(1.0, ref.abs().max().item()), "%s: off by %.3g (|ref| %.3g)" % (tag, err, ref.abs().max())


def run_all(case):
    """every entry point of the case against the one fp64 reference of its kind; each call must have run compact"""
    from pathnet_amd import _lib
    ro, remb, rpw, rps = case.oracle(train=False)
    _close("eval forward", case.eval_call(), ro)
    assert case.ran_compact(), "the eval forward did not run over compact rows"
    lo, emb, pw, ps = case.eval_call(encode=True)
    for tag, got, ref in (("encode logits", lo, ro), ("embedding", emb, remb), ("path weight", pw, rpw),
                          ("path state", ps, rps)):
        _close(tag, got, ref)
    b, n = case.S // 3, case.S // 3 + 1
    _close("group_slice", case.eval_call(group_slice=(b, n)), ro[b:b + n])
    assert case.ran_compact()
    rl, rout, rg = case.oracle(train=True)
    # (name, deterministic, fused, PN_POOL_STEP, micro-batches)
    modes = [("forward + backward", False, False, 1, False), ("forward + backward, deterministic", True, False, 1, False),
             ("fused, three launches", False, True, 0, False), ("fused, registers", False, True, 1, False),
             ("fused, pool_step", False, True, 2, False), ("fused, deterministic", True, True, 1, False)]
    if case.micro:
        modes += [("micro-batches, fused", False, True, 1, True), ("micro-batches, deterministic", True, False, 1, True)]
    for name, det, fused, knob, micro in modes:
        tag = "%s (PN_NODE_RGRAD=%d)" % (name, case.rgrad)
        old = _lib.set_knob("PN_POOL_STEP", knob)
        try:
            loss, out, grads = case.step(det, fused, micro)
        finally:
            _lib.set_knob("PN_POOL_STEP", old)
        assert case.ran_compact(), "%s: not compact" % tag
        _close(tag + ": logits", out, rout)
        assert abs(loss - rl) <= TOL * max(1.0, abs(rl)), "%s: loss %.9g, oracle %.9g" % (tag, loss, rl)
        try:
            assert_grads_close(grads, rg, zero_ok=case.zero_ok, tag=tag)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (tag, e)) from None


# auto: a shape where make_dims picks compact by itself (N = 20 000, 8 192 path steps against 80 000 rows); otherwise
# PN_COMPACT=1.  rgrad: PN_NODE_RGRAD of the case (compact rows: mmax = min(N, ZR) reduction rows).
CASES = {
    # library's own choice, rgrad_kernel with LIST + GATE at 8 192 rows (default knob), three micro-batches
    "homo_auto": dict(variant="homo", N=20000, S=256, W=8, auto=True, micro=100),
    # library's own choice, the atomic 64 x 64 GEMM over GEMM_IND_K, bf16 x 3 recurrence
    "hetero_auto_bf16x3": dict(variant="hetero", N=20000, S=256, W=8, auto=True, rgrad=0, math="bf16x3", micro=100),
    # library's own choice, RNN cell, rgrad_kernel (LIST, no gate)
    "pagg_auto": dict(variant="pagg", N=20000, S=256, W=8, H=64, auto=True),
    # segments of 63 / 64 / 65 rows, code 3 untouched; rgrad_kernel forced at 300 rows
    "homo_seg_63_64_65_none": dict(variant="homo", N=300, S=40, W=8, paths="sizes", sizes=(63, 64, 65, 0), rgrad=2),
    "pagg_seg_63_64_65_none": dict(variant="pagg", N=300, S=40, W=8, H=64, paths="sizes", sizes=(64, 0, 65, 63), rgrad=0),
    # segments of 127 / 128 / 129 rows and one of a single row
    "hetero_seg_127_128_129_1": dict(variant="hetero", N=300, S=40, W=8, paths="sizes", sizes=(127, 128, 129, 1), rgrad=2,
                                     micro=14),
    "homo_gru_seg_129_1_128_127": dict(variant="homo", N=300, S=40, W=8, cell="gru", paths="sizes",
                                       sizes=(129, 1, 128, 127), rgrad=1),
    # every (node, code) row touched (ZR == N * L); N * L = 141: odd, scalar tail of scan_count_kernel
    "homo_gru_bf16x3_all_odd": dict(variant="homo", N=47, S=30, W=6, L=3, cell="gru", math="bf16x3", paths="all", rgrad=2),
    "pagg_all_tail": dict(variant="pagg", N=45, S=30, W=6, H=32, paths="all", rgrad=0),       # N * L = 180 = 11 * 16 + 4
    "hetero_all": dict(variant="hetero", N=61, S=24, W=5, L=5, paths="all", rgrad=2, micro=9),  # 305 rows
    # one touched row: every step is (N - 1, L - 2), every dZ contribution lands on one row
    "homo_one_row": dict(variant="homo", N=90, S=20, W=6, paths="one", rgrad=2),
    "hetero_mean_H100_one_row": dict(variant="hetero", N=90, S=20, W=6, H=100, cell="mean", paths="one", rgrad=1),
    # the generic recurrence (H > 256), nodes 0 and N - 1 at every code
    "homo_gru_H288_ends": dict(variant="homo", N=200, S=30, W=6, H=288, cell="gru", paths="ends", rgrad=2, micro=11),
    # padded hidden size, mean cell, nodes 0 and N - 1 at every code
    "homo_mean_H100_ends": dict(variant="homo", N=200, S=30, W=6, H=100, cell="mean", paths="ends", rgrad=0),
}


def _force_compact(monkeypatch, auto):
    if auto:
        monkeypatch.delenv("PN_COMPACT", raising=False)
    else:
        monkeypatch.setenv("PN_COMPACT", "1")


def _rgrad(request, value):
    from pathnet_amd import _lib
    old = _lib.set_knob("PN_NODE_RGRAD", value)
    request.addfinalizer(lambda: _lib.set_knob("PN_NODE_RGRAD", old))


@pytest.mark.parametrize("name", sorted(CASES))
def test_compact_rows_match_the_fp64_oracle(name, monkeypatch, request):
    cfg = CASES[name]
    _force_compact(monkeypatch, cfg.get("auto", False))
    _rgrad(request, cfg.get("rgrad", 1))
    run_all(Case(**cfg))


def test_rows_left_by_a_larger_call_are_not_read(monkeypatch, request):
    """One module, one workspace: a batch that touches many rows (a spike node among them, forced fp16 x 2), then a batch
    of the same shape that touches three rows per code -- rows past its seg[L] still hold the first call's Z / dZ (and the
    spike's magnitude).  The second call alone matches fp64, eval and training; then a dense eval forward that may reuse
    the tables (reuse_tables) after the compact one matches too."""
    from pathnet_amd import modules as M
    monkeypatch.setenv("PN_COMPACT", "1")
    _rgrad(request, 2)
    big = Case("homo", N=400, S=40, W=8, paths="ends", math="f16x2", seed=5)
    big.X[big.sets[3][1]] *= 2.0 ** 30
    small = Case("homo", N=400, S=40, W=8, paths="sizes", sizes=(3, 3, 3, 3), seed=6)
    small.m, small.X = big.m, big.X
    assert big.sets[3][1] not in np.concatenate(small.sets) and big.sets[3][1] not in small.sel
    big.eval_call()
    big.step(False, False)
    assert big.ran_compact()
    _close("second eval", small.eval_call(), small.oracle(train=False)[0])
    rl, rout, rg = small.oracle(train=True)
    for det in (False, True):
        big.step(det, True)
        loss, out, grads = small.step(det, True)
        assert small.ran_compact()
        _close("second training call", out, rout)
        assert abs(loss - rl) <= TOL * max(1.0, abs(rl))
        assert_grads_close(grads, rg, tag="second training call, deterministic=%s" % det)
    # the eval workspace now holds the small batch's compact rows: a dense call must compute the whole bank again
    small.eval_call()
    monkeypatch.setenv("PN_COMPACT", "0")
    small.m.seq_math = "bf16x3"         # (the dense bank holds the spike's rows: beyond the fp16 x 2 window)
    ids, codes, sel, _ = small.dev
    with torch.no_grad():
        out = small.m(small.X.cuda(), ids, small.W, small.L, sel, codes, None, reuse_tables=True).cpu().double()
    assert not M.shape_info(small.m._last_shape[0])[0]
    _close("dense call after compact", out, small.oracle(train=False)[0])


def test_spike_row_among_the_touched_rows_falls_back_to_bf16x3(monkeypatch):
    """launch_range_rows reads the spread of Z over the seg[L] compact rows.  A node whose feature row is 2^40 times the
    typical one is touched at the highest code only, as the LAST compact row (node N - 1): the range guard must see it, re-run the call in
    bf16 x 3 and return the fp64 result -- a count short of seg[L] leaves the spike out and the f16 x 2 result is wrong."""
    import warnings
    monkeypatch.setenv("PN_COMPACT", "1")
    case = Case("homo", N=300, S=40, W=8, paths="last", sizes=(90, 70, 80, 60), seed=9)
    assert case.sets[3][-1] == case.N - 1 and all(case.N - 1 not in r for r in case.sets[:3]) and case.N - 1 not in case.sel
    case.X[case.N - 1] *= 2.0 ** 40
    want = case.oracle(train=False)[0]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = case.eval_call()
    assert case.ran_compact()
    assert case.m._range_wide and any("bf16x3" in str(x.message) for x in w)
    _close("spike among the compact rows", out, want)
