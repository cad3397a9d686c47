"""The sparse fc0 route (pathnet_amd/csrc/pn_sparse.hip) at the edges its own constants set -- 4096 counts per scan round, 64
stored entries per chunk, 8 per group, 4 wavefronts per column, 64 rows per bias block, NJ = ceil(H / 64) columns per lane --
against np.nonzero (structure, exact) and the fp64 restatement with the derived per-element bound of tests/sparse_fc0_ref.py
(values).  tests/test_gpu_sparse_fc0.py stays what it is: the route through the whole model, at 67 x 13 and 130 x 129.

The handle on the kernels.  encode() returns embedding[:, :H] = Xh[sel] and is differentiable.  With every node selected
(sel = arange(N)), W = L = 1, no dropout and sparse_features = "always", embedding[:, :H] is the forward kernel's output for EVERY
row, and the loss (embedding[:, :H] * R).sum() makes dXh = R exactly (the logits and the pooled half receive no gradient), so
fc0.weight.grad and fc0.bias.grad are the weight-gradient kernel's output for EVERY column and the bias blocks' (deterministic
mode: colsum's) from operands the test knows.  That closes "rows the batch does not touch": through the whole model only the 20
masked nodes' logits were compared, a wrong Xh row of a node no path visits reached nothing, and a wrong g_fc0_w entry was judged
against |g|_inf of the whole tensor; here every element has its own bound.  PathNet runs the kernels without ReLU and with
gate = nullptr, PathNet_homo with the ReLU forward and the gated backward; for the latter the reference takes its gate from the
GPU's own Xh > 0, which the same test has just held to fp64 (a pre-activation within rounding of zero may fall on either side).
Every value case prints its largest error / bound for Xh, g_w and g_b (pytest -s)."""
import ctypes

import numpy as np
import pytest
import torch

import sparse_fc0_ref as sr

pytestmark = pytest.mark.gpu

C = 3


def _cls(variant):
    import pathnet_amd
    return {"homo": pathnet_amd.PathNet_homo, "hetero": pathnet_amd.PathNet}[variant]


# ---- structure ------------------------------------------------------------------------------------------------------------------
def assert_structure_equals_numpy_nonzero(x):
    """tests/test_gpu_sparse_fc0.py's structure assertions, restated for any fp32 matrix x"""
    from pathnet_amd import modules
    N, F = x.shape
    feat = modules.PreparedFeatures(torch.tensor(x).cuda()).fill()
    torch.cuda.synchronize()
    bits = x.view(np.int32)
    r, c = np.nonzero(x)                                    # row-major: rows ascend, features ascend inside a row
    row_off = feat.row_off.cpu().numpy()
    col_off = feat.col_off.cpu().numpy()
    assert feat.nnz == len(r) == row_off[N] == col_off[F]
    assert (row_off == np.concatenate([[0], np.cumsum(np.bincount(r, minlength=N))])).all()
    assert (feat.col.cpu().numpy() == c).all()
    assert (feat.val.cpu().numpy().view(np.int32) == bits[r, c]).all()
    c2, r2 = np.nonzero(x.T)                                # column-major: features ascend, nodes ascend inside a column
    assert (col_off == np.concatenate([[0], np.cumsum(np.bincount(c2, minlength=F))])).all()
    assert (feat.row.cpu().numpy() == r2).all()
    assert (feat.valc.cpu().numpy().view(np.int32) == bits[r2, c2]).all()
    return row_off, col_off


SCAN_PAIRS = [(1, 1), (2, 63), (4, 64), (5, 65), (255, 1025), (256, 1023), (257, 1024), (4095, 65), (4096, 64), (4097, 5),
              (8191, 2), (8192, 4), (8193, 3), (12289, 1)]
SCAN_SHAPES = sorted(set(SCAN_PAIRS) | {(F, N) for N, F in SCAN_PAIRS})


@pytest.mark.parametrize("N,F", SCAN_SHAPES)
def test_offsets_and_entries_equal_numpy_nonzero_at_every_scan_length(N, F):
    """sp_scan_kernel, everything past its first three wavefronts: offsets arrays of more than 130 counts; more than 256 counts,
    from which the sum over earlier wavefronts (`before`) is non-zero; exactly 4096 counts, a full round; more than 4096, where
    `carry` enters a second round (and a third: 8193, 12289) -- each as the rows' array and, transposed, as the columns', and each
    checked against np.nonzero, which no shape larger than 130 was.  (Pubmed has N = 19 717 and Citeseer F = 3 703: real data
    takes these paths; the 2708 x 64 matrices of the eligibility tests were never compared with anything.)  About 30 % of the
    entries are stored, some rows and columns hold none."""
    assert_structure_equals_numpy_nonzero(sr.structure_matrix(N, F))


def test_scan_carries_a_large_sum_into_its_second_round():
    """4097 rows whose last one, the single count of the scan's second round, is full: `carry` is 600 there, so losing it costs
    600 positions and not an off-by-few, and every entry of the row (most of the matrix) would land in the wrong place"""
    row_off, _ = assert_structure_equals_numpy_nonzero(sr.carry_matrix())
    assert row_off[4096] == 600 and row_off[4097] == 1500


# ---- values ---------------------------------------------------------------------------------------------------------------------
def run_kernels(variant, name, N, H, det=False, model=None):
    """one forward and backward through the handle -> (Xh [N, H], g_w [H, F], g_b [H]) as numpy, the module, and the padded
    operands' gradients (g_w [Hk, F], g_b [Hk]) when the module pads H, else None"""
    X, W, b, R = sr.operands(name, N, H)
    n, F = X.shape
    m = model
    if m is None:
        m = _cls(variant)(F, H, C, 1, dropout=0.0)
        with torch.no_grad():
            m.fc0.weight.copy_(torch.tensor(W))
            m.fc0.bias.copy_(torch.tensor(b))
        m = m.cuda().train()
    m.sparse_features, m.deterministic = "always", det
    kept = []
    if H % 32:      # the zero-padded fc0 operands are functions of the parameters inside the call: keep their gradients
        inner = type(m)._padded_param_inputs

        def keeping(Hk):
            fw, fb, params = inner(m, Hk)
            for t in params[:2]:
                t.retain_grad()
            kept[:] = params[:2]
            return fw, fb, params
        m._padded_param_inputs = keeping
    m.zero_grad(set_to_none=True)
    calls = dict(m.fc0_route_calls)
    ids = torch.arange(n, dtype=torch.int32).reshape(n, 1).cuda()
    sel = torch.arange(n, dtype=torch.int32).cuda()
    codes = torch.zeros(n, 1, 1, dtype=torch.uint8).cuda()
    enc = m.encode(torch.tensor(X).cuda(), ids, 1, 1, sel, codes, None)
    assert m.fc0_route == "sparse" and m.fc0_route_calls == {"sparse": calls["sparse"] + 1, "dense": 0}
    assert enc.embedding.shape == (n, 2 * H)
    Xh = enc.embedding[:, :H]
    (Xh * torch.tensor(R).cuda()).sum().backward()
    torch.cuda.synchronize()
    got = tuple(t.detach().cpu().numpy().copy() for t in (Xh, m.fc0.weight.grad, m.fc0.bias.grad))
    padded = tuple(t.grad.detach().cpu().numpy().copy() for t in kept) if kept else None
    return got, m, padded


def check_against_fp64(variant, name, N, H, got, label=""):
    """every element of Xh, g_w and g_b inside its own derived bound; prints the largest error / bound of each first"""
    X, W, b, R = sr.operands(name, N, H)
    Xh, g_w, g_b = got
    relu = variant == "homo"
    fwd = sr.reference(X, W, b, R, relu)
    ref = sr.reference(X, W, b, R, relu, gate=(Xh > 0) if relu else None)
    worst = {k: float(sr.ratio(g, ref[k], ref["bound_" + k]).max()) for k, g in (("Xh", Xh), ("g_w", g_w), ("g_b", g_b))}
    print("sparse fc0 edges %s %s N=%d F=%d H=%d%s: error / bound  Xh %.3f  g_w %.3f  g_b %.3f"
          % (variant, name, X.shape[0], X.shape[1], H, label, worst["Xh"], worst["g_w"], worst["g_b"]))
    assert Xh.shape == fwd["Xh"].shape and g_w.shape == ref["g_w"].shape and g_b.shape == ref["g_b"].shape
    assert worst["Xh"] <= 1.0, worst
    # a row without a stored entry is act(bias), to the bit; a column without one gets an exactly-zero gradient
    act_b = np.maximum(b, 0.0) if relu else b
    assert (Xh[~(X != 0).any(1)].view(np.int32) == act_b.view(np.int32)).all()
    assert not g_w[:, ~(X != 0).any(0)].any()
    assert worst["g_w"] <= 1.0 and worst["g_b"] <= 1.0, worst
    return worst


VARIANTS = ["hetero", "homo"]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("H", [32, 128])
def test_row_staircase_every_row_length_of_the_forward(variant, H):
    """Forward row lengths: row n of the 200 x 136 matrix holds exactly n stored entries for n = 0 .. 136, the other rows repeat
    63, 64, 65, 71, 72, 73, 127, 128, 129, 136.  That runs a last chunk of exactly 8 entries (rows of 8, 72, 136: no short group)
    and of 9 (rows of 9, 73: a group of one), rows of 63, 64 and 65 entries (one chunk short of full, full, full plus one lane),
    and every group remainder 1 .. 7 -- where only 0, ~6, ~78 and 129 stored entries occurred before."""
    got, _, _ = run_kernels(variant, "rows", None, H)
    check_against_fp64(variant, "rows", None, H, got)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "deterministic"])
@pytest.mark.parametrize("H", [32, 128])
def test_column_staircase_every_column_length_of_the_weight_gradient(variant, H, det):
    """sparse_fc0_wgrad_kernel, the second trip of its `i0` loop: a wavefront sums every fourth entry of a column, so the trip
    needs a column of more than 256 stored entries, and N <= 130 capped that at 33 per wavefront.  The 530 x 72 matrix has columns
    of exactly 0 .. 5, 7, 8, 9, 31 .. 37 (wavefronts with and without a short group), 255, 256, 257, 259, 260, 261 (the last
    wavefront to stay in one trip, the first to enter the second, one after the other), 511 .. 520 and 530 (two full trips and
    a third).  sparse_bias_block: 530 rows end in a last block of 18 rows, in which wavefronts 2 and 3 have no row; the default mode
    runs the bias blocks' atomics, the deterministic mode colsum, and there a second run repeats the bits."""
    got, m, _ = run_kernels(variant, "cols", None, H, det=det)
    check_against_fp64(variant, "cols", None, H, got, " det" if det else "")
    if det:
        again, _, _ = run_kernels(variant, "cols", None, H, det=True, model=m)
        for a, b in zip(got, again):
            assert (a.view(np.int32) == b.view(np.int32)).all()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("H", sr.HIDDEN_SIZES)
def test_every_hidden_size_of_the_column_groups(variant, H):
    """NJ = 1 .. 4 at every multiple of 32: NJ = 3 (H = 160, 192) was never instantiated by a test, and the partly filled last
    column group (`h < H` with H = 96, 160, 224) never ran.  A padded hidden size never took the sparse route in a test: H = 40
    and 100 run the kernels at 64 and 128 and are compared at the module's own H; the padded units' gradients, which autograd
    drops on the way to the parameters, are read off the padded operands and must be exactly zero."""
    got, _, padded = run_kernels(variant, "hidden", None, H)
    check_against_fp64(variant, "hidden", None, H, got)
    assert (padded is not None) == (H in (40, 100))
    if padded is not None:
        Hk = -(-H // 32) * 32
        pw, pb = padded
        assert pw.shape == (Hk, 40) and pb.shape == (Hk,)
        assert not pw[H:].any() and not pb[H:].any()
        assert (pw[:H].view(np.int32) == got[1].view(np.int32)).all() and (pb[:H].view(np.int32) == got[2].view(np.int32)).all()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("N", sr.NODE_COUNTS)
def test_node_counts_of_the_bias_blocks_and_the_row_grids(variant, N):
    """sparse_bias_block and the one-wavefront-per-row grids at N = 1; N < 16, where only wavefront 0 of the bias block has live
    rows (3, 15); 16 and 17, the first row of wavefront 1; 63 and 65 around a block; N an exact multiple of 64 (64, 128: no
    partial block) -- a last block in which some wavefronts have no row (17: wavefronts 2, 3; 65: 1, 2, 3).  F = 9, H = 64."""
    got, _, _ = run_kernels(variant, "nodes", N, 64)
    check_against_fp64(variant, "nodes", N, 64, got)


@pytest.mark.parametrize("variant", VARIANTS)
def test_rows_beyond_one_scan_round_carry_values(variant):
    """N = 4100 > 4096 with values: the rows past the scan's first round are stored and compared like all the others, element
    by element -- a scan error at row 4097 would have gone unnoticed through the whole model even if that shape had been run."""
    got, _, _ = run_kernels(variant, "round", None, 32)
    worst = check_against_fp64(variant, "round", None, 32, got)
    X, W, b, R = sr.operands("round", None, 32)
    tail = sr.reference(X, W, b, R, variant == "homo")
    assert sr.ratio(got[0][4096:], tail["Xh"][4096:], tail["bound_Xh"][4096:]).max() <= 1.0 and worst["Xh"] <= 1.0


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["empty", "single"])
def test_no_stored_entry_and_a_single_one_in_the_last_corner(variant, name):
    """67 x 13 without a stored entry, and with one at (N - 1, F - 1): the forward equals the bias (with ReLU for homo) to the
    bit, g_w is exactly zero apart from the one column"""
    got, _, _ = run_kernels(variant, name, None, 64)
    check_against_fp64(variant, name, None, 64, got)
    X, W, b, R = sr.operands(name, None, 64)
    Xh, g_w, _ = got
    act_b = np.maximum(b, 0.0) if variant == "homo" else b
    assert (Xh[:66].view(np.int32) == act_b.view(np.int32)).all()
    assert not g_w[:, :12].any()
    if name == "empty":
        assert (Xh[66].view(np.int32) == act_b.view(np.int32)).all() and not g_w.any()
    else:
        assert (Xh[66] != act_b).any() and g_w[:, 12].any()


# ---- eligibility at its thresholds ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,nnz,want,scans", [(2047, 1300, "dense", 0), (2048, 1300, "sparse", 1), (2048, 2048, "sparse", 1),
                                              (2048, 2049, "dense", 1)])
def test_auto_mode_at_the_node_floor_and_the_density_threshold(N, nnz, want, scans):
    """sparse_features = "auto", F = 64, eval forwards (as test_auto_mode_prepares_large_sparse_matrices_only): N = 2047 is never
    scanned, N = 2048 is; at N = 2048, nnz = N * F / 64 exactly takes the sparse route (the test in the code is `>`), one more
    entry the dense one"""
    import pathnet_amd
    F, S, W, L = 64, 20, 3, 4
    torch.manual_seed(N + nnz)
    m = pathnet_amd.PathNet_homo(F, 32, 5, L, dropout=0.0).cuda().eval()
    assert m.sparse_features == "auto" and m.sparse_min_nodes == 2048 and m.sparse_max_density == 1 / 64
    g = torch.Generator().manual_seed(N + nnz)
    X = torch.zeros(N * F)
    X[torch.randperm(N * F, generator=g)[:nnz]] = 1.0
    X = X.view(N, F).cuda()
    assert int(torch.count_nonzero(X).item()) == nnz and (nnz == 2048) == (nnz * 64 == N * F)
    ids = torch.randint(0, N, (S, W * L), generator=g).to(torch.int32).cuda()
    sel = torch.arange(S, dtype=torch.int32).cuda()
    codes = torch.randint(0, L, (S, W, L), generator=g).to(torch.uint8).cuda()
    key = (X.data_ptr(), (N, F), int(X._version), X.device)
    with torch.no_grad():
        for _ in range(2):
            m(X, ids, W, L, sel, codes, None)
            assert m.fc0_route == want
    assert m.fc0_route_calls == {want: 2, {"dense": "sparse", "sparse": "dense"}[want]: 0}
    assert m.sparse_scans == scans
    assert list(m._sparse_cache) == ([key] if want == "sparse" else [])
    assert list(m._sparse_dense) == ([key] if (want == "dense" and scans) else [])


@pytest.mark.parametrize("what", ["count_null_offsets", "count_N_0", "count_F_0", "fill_null_features", "fill_null_col"])
def test_entry_points_refuse_bad_arguments_without_a_launch(what):
    from pathnet_amd import _lib
    lib, ctx = _lib.load(), _lib.context("cuda")
    X = torch.ones(8, 8, device="cuda")
    off = torch.full((9,), -7, dtype=torch.int32, device="cuda")
    one = torch.zeros(64, dtype=torch.int32, device="cuda")
    if what == "count_null_offsets":
        rcs = [lib.pn_sparse_count(ctx, X.data_ptr(), 8, 8, None, off.data_ptr(), None),
               lib.pn_sparse_count(ctx, X.data_ptr(), 8, 8, off.data_ptr(), None, None)]
    elif what == "count_N_0":
        rcs = [lib.pn_sparse_count(ctx, X.data_ptr(), 0, 8, off.data_ptr(), off.data_ptr(), None)]
    elif what == "count_F_0":
        rcs = [lib.pn_sparse_count(ctx, X.data_ptr(), 8, 0, off.data_ptr(), off.data_ptr(), None)]
    elif what == "fill_null_features":
        rcs = [lib.pn_sparse_fill(ctx, X.data_ptr(), 8, 8, None, None)]
    else:
        sp = _lib.SparseFeatures(64, off.data_ptr(), None, one.data_ptr(), off.data_ptr(), one.data_ptr(), one.data_ptr())
        rcs = [lib.pn_sparse_fill(ctx, X.data_ptr(), 8, 8, ctypes.byref(sp), None)]
    torch.cuda.synchronize()
    assert rcs == [_lib.PN_ERR_ARG] * len(rcs)
    assert (off.cpu() == -7).all() and not one.any()        # nothing was launched: the arrays are as they were
