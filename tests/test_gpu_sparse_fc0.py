"""fc0 over prepared sparse features (pathnet_amd/csrc/pn_sparse.hip; module attribute `sparse_features`).

Structure: the CSR and CSC indexes pn_sparse_count / pn_sparse_fill build equal np.nonzero of X exactly, in order.
Values: logits and the fc0 gradients of the sparse route against the fp64 restatement of the reference (oracle/pagg_oracle.py),
with the bound of tests/test_gpu_grad_error.py -- every error at most max(8 x the fp32 oracle's own error, 2e-6 x |g|_inf),
logits within 2e-6 -- and the dense route ("never") inside tests/gradcheck.py's default bound of the sparse one.
The cases are small (N = 67 with F = 13: a dense bank and the fp16 range words cleared by the sparse launch; N = 130 with
F = 129: compact rows, more than one 64-wide chunk of features).  Neither kernel has a size threshold: a wavefront owns a node, a
workgroup a feature; the "thick" cases give every wavefront of a column more than one group of eight entries."""
import functools

import numpy as np
import pytest
import torch
from gradcheck import ZERO_OK_HETERO, assert_grads_close

from oracle import pagg_oracle as po

pytestmark = pytest.mark.gpu

C, S, W, L = 5, 20, 3, 4


def _cls(variant):
    import pathnet_amd
    return {"homo": pathnet_amd.PathNet_homo, "hetero": pathnet_amd.PathNet}[variant]


def make_X(kind, N, F, seed=0):
    """CPU fp32 [N, F].  rand: ~5 % non-zeros with values in [0.5, 1.5) / row count; the others are the edge cases by name."""
    g = torch.Generator().manual_seed(1000 + seed)
    X = (torch.rand(N, F, generator=g) < 0.05).float() * (0.5 + torch.rand(N, F, generator=g))
    if kind == "empty":             # an empty row and an empty column
        X[3, :] = 0.0
        X[:, 5] = 0.0
    elif kind == "full":            # a full row, and a full column: N entries, every wavefront of its workgroup gets several
        X[7, :] = 0.5 + torch.rand(F, generator=g)
        X[:, 11] = 0.5 + torch.rand(N, generator=g)
    elif kind == "zero":
        X.zero_()
    elif kind == "single":
        X.zero_()
        X[N - 1, F - 1] = 0.75
    elif kind == "negzero":         # -0.0f is no non-zero
        X[X == 0.0] = -0.0
        assert bool(torch.signbit(X).any())
    elif kind == "thick":           # 60 % non-zeros: ~78 entries a column, ~20 a wavefront (more than one group of eight), rows of several groups
        X = (torch.rand(N, F, generator=g) < 0.6).float() * (0.5 + torch.rand(N, F, generator=g))
    elif kind == "nonfinite":       # NaN and Inf are (structure only)
        X[2, 1], X[4, 0], X[N - 1, 2] = float("nan"), float("inf"), float("-inf")
    else:
        assert kind == "rand"
    if kind != "nonfinite":
        X = X / X.sum(1, keepdim=True).clamp(min=1.0)
    return X.contiguous()


# ---- structure --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N,F", [("rand", 67, 13), ("rand", 130, 129), ("empty", 130, 129), ("full", 130, 129),
                                      ("zero", 67, 13), ("single", 130, 129), ("negzero", 67, 13), ("nonfinite", 67, 13)])
def test_csr_and_csc_equal_numpy_nonzero_in_order(kind, N, F):
    from pathnet_amd import modules
    X = make_X(kind, N, F)
    feat = modules.PreparedFeatures(X.cuda()).fill()
    torch.cuda.synchronize()
    x = X.numpy()
    bits = x.view(np.int32)
    r, c = np.nonzero(x)                                    # row-major: rows ascend, features ascend inside a row
    assert feat.nnz == len(r)
    if kind == "negzero":
        assert feat.nnz < (bits != 0).sum()                 # the -0.0f entries have bits set and are not stored
    row_off = feat.row_off.cpu().numpy()
    assert (row_off == np.concatenate([[0], np.cumsum(np.bincount(r, minlength=N))])).all()
    assert (feat.col.cpu().numpy() == c).all()
    assert (feat.val.cpu().numpy().view(np.int32) == bits[r, c]).all()
    c2, r2 = np.nonzero(x.T)                                # column-major: features ascend, nodes ascend inside a column
    col_off = feat.col_off.cpu().numpy()
    assert (col_off == np.concatenate([[0], np.cumsum(np.bincount(c2, minlength=F))])).all()
    assert (feat.row.cpu().numpy() == r2).all()
    assert (feat.valc.cpu().numpy().view(np.int32) == bits[r2, c2]).all()
    if kind == "full":
        assert col_off[12] - col_off[11] == N and row_off[8] - row_off[7] == F


def test_count_refuses_more_than_2_pow_28_elements():
    from pathnet_amd import _lib
    X = torch.zeros(8, device="cuda")
    off = torch.zeros(8, dtype=torch.int32, device="cuda")
    rc = _lib.load().pn_sparse_count(_lib.context("cuda"), X.data_ptr(), 1 << 15, (1 << 13) + 1, off.data_ptr(), off.data_ptr(), None)
    assert rc == _lib.PN_ERR_ARG


# ---- values -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(variant, H, kind, N, F):
    """inputs, initial parameters and the oracle's results (fp64 and fp32) of a case: computed once, shared, never modified"""
    seed = 7 * H + F
    torch.manual_seed(seed)
    state = {k: v.detach().clone() for k, v in _cls(variant)(F, H, C, L, dropout=0.0).state_dict().items()}
    rng = np.random.default_rng(seed)
    X = make_X(kind, N, F, seed)
    sel = np.sort(rng.choice(N, S, replace=False))
    ids = rng.integers(0, N, (S, W, L)).astype(np.int32)
    ids[:, :, 0] = sel[:, None]
    codes = rng.integers(0, L, (S, W, L)).astype(np.uint8)
    y = torch.as_tensor(rng.integers(0, C, S))
    ref = {}
    for dt in (torch.float64, torch.float32):
        params = {k: v.to(dt).clone().requires_grad_(True) for k, v in state.items()}
        o = po.forward(variant, params, X, ids, codes, sel, W, L, dtype=dt)
        torch.nn.functional.cross_entropy(o, y).backward()
        ref[dt] = (o.detach().double(), {k: p.grad.double() for k, p in params.items() if p.grad is not None})
    return dict(variant=variant, H=H, F=F, state=state, X=X, sel=sel, ids=ids, codes=codes, y=y, ref=ref)


def run_gpu(case, mode, det=False, x_grad=False, X=None, model=None):
    """one training step of a fresh module with the case's parameters -> (logits, {name: gradient}, module, X on the GPU)"""
    m = model
    if m is None:
        m = _cls(case["variant"])(case["F"], case["H"], C, L, dropout=0.0)
        m.load_state_dict(case["state"])
        m = m.cuda().train()
    m.sparse_features, m.deterministic = mode, det
    X = case["X"].cuda() if X is None else X
    if x_grad:
        X.requires_grad_()
    m.zero_grad(set_to_none=True)
    out = m(X, torch.as_tensor(case["ids"].reshape(S, W * L)).cuda(), W, L, torch.as_tensor(case["sel"].astype(np.int32)).cuda(),
            torch.as_tensor(case["codes"]).cuda(), None)
    torch.nn.functional.cross_entropy(out, case["y"].cuda()).backward()
    torch.cuda.synchronize()
    grads = {k: v.grad.detach().clone() for k, v in m.named_parameters()}
    return out.detach().clone(), grads, m, X


VALUE_CASES = ([(v, H, "rand", N, F) for v in ("homo", "hetero") for H in (32, 128, 256) for N, F in ((67, 13), (130, 129))] +
               [(v, 128, kind, 130, 129) for v in ("homo", "hetero") for kind in ("empty", "full", "zero", "single", "negzero")] +
               [(v, H, "thick", 130, 13) for v in ("homo", "hetero") for H in (128, 256)])


@pytest.mark.parametrize("variant,H,kind,N,F", VALUE_CASES)
def test_sparse_route_against_the_fp64_oracle_and_the_dense_route(variant, H, kind, N, F):
    case = reference(variant, H, kind, N, F)
    out, grads, m, _ = run_gpu(case, "always")
    assert m.fc0_route == "sparse" and m.fc0_route_calls["dense"] == 0
    exact_out, exact = case["ref"][torch.float64]
    _, f32 = case["ref"][torch.float32]
    out_err = (out.cpu().double() - exact_out).abs().max().item()
    print("logits max abs err %.3e" % out_err)
    rows = {}
    for k in ("fc0.weight", "fc0.bias"):
        rows[k] = ((grads[k].cpu().double() - exact[k]).abs().max().item(), (f32[k] - exact[k]).abs().max().item(),
                   exact[k].abs().max().item())
        print("%s: hip err %.3e  torch fp32 err %.3e  |g|_inf %.3e" % ((k,) + rows[k]))
    assert out_err < 2e-6
    for k, (err, err32, ginf) in rows.items():
        assert err <= max(8.0 * err32, 2e-6 * ginf), (k, err, err32, ginf)
    out_d, grads_d, m_d, _ = run_gpu(case, "never")
    assert m_d.fc0_route == "dense" and m_d.fc0_route_calls["sparse"] == 0
    assert (out_d - out).abs().max().item() < 4e-6          # (two results, each within 2e-6 of the exact one)
    assert_grads_close(grads_d, grads, zero_ok=ZERO_OK_HETERO if variant == "hetero" else ())


@pytest.mark.parametrize("variant", ["homo", "hetero"])
def test_deterministic_mode_takes_the_sparse_route_and_repeats_its_bits(variant):
    case = reference(variant, 128, "full", 130, 129)
    out0, g0, m, X = run_gpu(case, "always", det=True)
    assert m.fc0_route == "sparse"
    out1, g1, _, _ = run_gpu(case, "always", det=True, X=X, model=m)
    assert m.fc0_route_calls == {"sparse": 2, "dense": 0}
    assert torch.equal(out0, out1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    _, g2, _, _ = run_gpu(case, "always")                   # the default (atomic) backward agrees within the parity tolerance
    assert_grads_close(g0, g2, zero_ok=ZERO_OK_HETERO if variant == "hetero" else ())


def test_gradient_of_X_stays_the_dense_gemm():
    case = reference("homo", 128, "rand", 130, 129)
    _, _, m, Xs = run_gpu(case, "always", x_grad=True)
    _, _, md, Xd = run_gpu(case, "never", x_grad=True)
    assert m.fc0_route == "sparse" and md.fc0_route == "dense"
    assert_grads_close({"X": Xs.grad}, {"X": Xd.grad})


def test_in_place_change_of_X_rebuilds_the_features():
    case = reference("homo", 128, "rand", 130, 129)
    out1, _, m, X = run_gpu(case, "always")
    with torch.no_grad():
        X.mul_(2.0)
    out2, _, _, _ = run_gpu(case, "always", X=X, model=m)
    assert m.fc0_route == "sparse" and len(m._sparse_cache) == 2          # (a new key: the version counter moved)
    params = {k: v.double() for k, v in case["state"].items()}
    want = po.forward("homo", params, case["X"] * 2.0, case["ids"], case["codes"], case["sel"], W, L, dtype=torch.float64)
    assert (want - out1.cpu().double()).abs().max().item() > 1e-3         # the inputs: doubling X moves the logits
    assert (want - out2.cpu().double()).abs().max().item() < 2e-6


def _graph_step(case, m, X):
    ids = torch.as_tensor(case["ids"].reshape(S, W * L)).cuda()
    sel = torch.as_tensor(case["sel"].astype(np.int32)).cuda()
    codes = torch.as_tensor(case["codes"]).cuda()
    y = case["y"].cuda()
    params = list(m.parameters())

    def step(X=X):
        out = m(X, ids, W, L, sel, codes, None)
        return [out] + list(torch.autograd.grad(torch.nn.functional.cross_entropy(out, y), params))
    return step


def _graph_module(case):
    m = _cls(case["variant"])(case["F"], case["H"], C, L, dropout=0.0)
    m.load_state_dict(case["state"])
    m = m.cuda().train()
    m.sparse_features, m.deterministic = "always", True
    m.range_guard = False           # (its read-backs are host round trips; a capture has none)
    return m


def _warm(step, *args):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            ref = step(*args)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    return [r.detach().clone() for r in ref]


def test_captured_step_with_a_seen_X_replays_the_eager_bits():
    case = reference("homo", 128, "rand", 130, 129)
    m = _graph_module(case)
    step = _graph_step(case, m, case["X"].cuda())
    ref = _warm(step)
    assert m.fc0_route == "sparse"
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = step()
    assert m.fc0_route == "sparse"
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(ref, got):
        assert torch.equal(a, b)


def test_captured_step_with_an_unseen_X_runs_dense_and_is_correct():
    case = reference("homo", 128, "rand", 130, 129)
    m = _graph_module(case)
    X1, X2 = case["X"].cuda(), case["X"].cuda()
    step = _graph_step(case, m, X1)
    _warm(step)                     # (X1 is prepared; X2 has not been seen)
    assert m.fc0_route == "sparse" and len(m._sparse_cache) == 1
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = step(X2)
    assert m.fc0_route == "dense" and len(m._sparse_cache) == 1            # not prepared, and nothing remembered
    graph.replay()
    torch.cuda.synchronize()
    got = [t.detach().clone() for t in got]
    exact_out, exact = case["ref"][torch.float64]
    assert (got[0].cpu().double() - exact_out).abs().max().item() < 2e-6
    ref = _warm(step, X2)           # eager, outside the capture: X2 is looked at now
    assert m.fc0_route == "sparse" and len(m._sparse_cache) == 2
    names = [k for k, _ in m.named_parameters()]
    assert_grads_close(dict(zip(names, got[1:])), dict(zip(names, ref[1:])))


# ---- eligibility: asserted through the module's route and scan counters -------------------------------------------------
def _small_batch(N, g):
    ids = torch.randint(0, N, (S, W * L), generator=g).to(torch.int32).cuda()
    sel = torch.arange(S, dtype=torch.int32).cuda()
    codes = torch.randint(0, L, (S, W, L), generator=g).to(torch.uint8).cuda()
    return ids, sel, codes


def _auto_module(F=64, H=32, seed=0):
    import pathnet_amd
    torch.manual_seed(seed)
    m = pathnet_amd.PathNet_homo(F, H, C, L, dropout=0.0).cuda().eval()
    assert m.sparse_features == "auto" and m.sparse_min_nodes == 2048 and m.sparse_max_density in (1 / 64, 1 / 32, 1 / 16)
    return m


@pytest.mark.parametrize("N,density,want", [(2708, None, "dense"), (2708, 0.013, "sparse"), (600, 0.013, "dense")])
def test_auto_mode_prepares_large_sparse_matrices_only(N, density, want):
    F = 64
    m = _auto_module(F, seed=N)
    g = torch.Generator().manual_seed(N)
    X = torch.rand(N, F, generator=g) if density is None else (torch.rand(N, F, generator=g) < density).float()
    X = X.cuda()
    ids, sel, codes = _small_batch(N, g)
    key = (X.data_ptr(), (N, F), int(X._version), X.device)
    with torch.no_grad():
        for _ in range(3):
            m(X, ids, W, L, sel, codes, None)
            assert m.fc0_route == want                              # from the first call on: two calls on one X take one route
    assert m.fc0_route_calls == {want: 3, {"dense": "sparse", "sparse": "dense"}[want]: 0}
    # looked at once; a matrix below the node floor is never looked at
    assert m.sparse_scans == (0 if N < 2048 else 1)
    assert list(m._sparse_cache) == ([key] if want == "sparse" else [])
    assert list(m._sparse_dense) == ([key] if (want == "dense" and N >= 2048) else [])


def test_fresh_or_changing_feature_tensors_stop_being_scanned():
    """What is not a resident matrix stops costing a count launch and a host read after two scans: a new tensor in every call
    (feature dropout, a gathered sub-matrix), a tensor changed in place between calls (learnable features).  Calls that compute a
    part of a batch (the runners of pathnet_amd.dist) are never scanned.  A resident matrix is still found afterwards."""
    from pathnet_amd import modules
    N, F = 2708, 64
    m = _auto_module(F, seed=5)
    g = torch.Generator().manual_seed(5)
    base = (torch.rand(N, F, generator=g) < 0.013).float().cuda()
    ids, sel, codes = _small_batch(N, g)
    with torch.no_grad():
        for _ in range(3):                      # a slice of the batch: dense, nothing looked at
            m(base, ids, W, L, sel, codes, None, group_slice=(0, S // 2))
        assert m.sparse_scans == 0 and m.fc0_route == "dense"
        for _ in range(8):
            X = base.clone()
            m(X, ids, W, L, sel, codes, None)
            del X
        assert m.sparse_scans == modules.SPARSE_MISS_LIMIT == 2
        X = base.clone()
        for _ in range(8):
            m(X, ids, W, L, sel, codes, None)
            X.add_(0.0)                         # same values, new version
        assert m.sparse_scans == modules.SPARSE_MISS_LIMIT and m.fc0_route == "dense"
        m(base, ids, W, L, sel, codes, None)    # the resident matrix: noted at its first sight now, looked at when it comes back
        assert m.sparse_scans == modules.SPARSE_MISS_LIMIT and m.fc0_route == "dense"
        for _ in range(2):
            m(base, ids, W, L, sel, codes, None)
            assert m.sparse_scans == modules.SPARSE_MISS_LIMIT + 1 and m.fc0_route == "sparse"
        m(base, ids, W, L, sel, codes, None, group_slice=(0, S // 2))
        assert m.fc0_route == "dense"


def test_prepared_entry_of_a_captured_graph_outlives_more_than_four_other_matrices():
    """A captured graph holds the device pointers of the features it was given: that entry is never evicted.  Other entries
    make room for new matrices, dense verdicts take no slot, and the replay still gives the eager bits afterwards."""
    from pathnet_amd import modules
    case = reference("homo", 128, "rand", 130, 129)
    m = _graph_module(case)
    X0 = case["X"].cuda()
    step = _graph_step(case, m, X0)
    ref = _warm(step)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = step()
    (key0, feat0), = m._sparse_cache.items()
    assert feat0.pinned
    ptrs = [t.data_ptr() for t in (feat0.row_off, feat0.col, feat0.val, feat0.col_off, feat0.row, feat0.valc)]
    others = [case["X"].cuda() * float(k + 2) for k in range(modules.SPARSE_CACHE_ENTRIES + 3)]
    for Xk in others:                           # seven more matrices through the same module, eagerly
        step(Xk)
    torch.cuda.synchronize()
    assert len(m._sparse_cache) == modules.SPARSE_CACHE_ENTRIES and m._sparse_cache[key0] is feat0
    assert [t.data_ptr() for t in (feat0.row_off, feat0.col, feat0.val, feat0.col_off, feat0.row, feat0.valc)] == ptrs
    m.sparse_features = "auto"                  # dense verdicts: remembered by key, no slot
    with torch.no_grad():
        for _ in range(2):
            step_dense = torch.rand(130, 129).cuda()
            m._sparse_dense[(step_dense.data_ptr(), (130, 129), 0, step_dense.device)] = True
    assert len(m._sparse_cache) == modules.SPARSE_CACHE_ENTRIES and key0 in m._sparse_cache
    for t in got:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(ref, got):
        assert torch.equal(a, b)
