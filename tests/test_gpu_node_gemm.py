"""The node-level GEMM entry points (pn_gemm_f32, pn_linear_forward, pn_linear_backward: pn_gemm.hip) held to EXACT
results at their tile, K-tail, split and dispatch edges, and the dense bank's gemm_kernel / gemm3_kernel line through the
aggregator.

Exact-integer operands.  A, B, bias, X, W, dY hold integers drawn uniformly from [-8, 8], stored as fp32.  Every product
is at most 64 in magnitude and every partial sum over K terms stays below K * 64 < 2^24 (asserted for every case before
any launch), so every fp32 product and every fp32 sum is exact in ANY order -- MFMA accumulation, split-K chunk sums,
atomicAdd, the fixed-order finish.  The expected result is the fp64 matmul (exact as well) cast to fp32 and the assertion
is torch.equal: a dropped, duplicated, misplaced or wrongly masked element fails outright and no tolerance is chosen.

Guards.  Every operand is a view inside a larger NaN-filled allocation (NaN before and after; for pn_gemm_f32, which
takes its strides freely, also NaN in the three pad elements of every leading dimension): a mask that lets a clamped or
neighbouring element through produces NaN.  Every output lives inside an allocation filled with a sentinel (-77); what
lies outside the M x N window -- the ldc - N pad columns, the floats before and after -- must still be the sentinel.

The routes, as pn_gemm.hip / pn_pagg.hip derive them (restated in fwd_chunks / bwd_chunks / colsum_blocks below, and held
to the case tables by the one CPU test of this file):
  * launch_gemm: 64 x 64 tiles, K tile 32.  Both operands K-contiguous, stored, one chunk, K <= 128 -> gemm_k128_kernel;
    everything else -> gemm_kernel<A layout, B layout, gate, row list>.
  * pn_linear_forward (launch_gemm_split): nz = min(8, ceil(512 / tiles), K // 64) with tiles = ceil(rows / 64) *
    ceil(out_f / 64); nz <= 1 or no (or a too small) workspace -> one launch_gemm; else the chunk length is ceil(K / nz)
    rounded up to 32, nz is recomputed as ceil(K / chunk), the chunk sums go to the workspace and gemm_finish_kernel adds
    them in chunk order (+ bias, ReLU).
  * pn_linear_backward: g_W = dY^T . X reduces over `rows` in ceil(rows / 256) chunks (at most 32 in the workspace
    route), chunk length rounded up to 32 and the count recomputed; without a workspace the chunks meet in atomicAdd, with
    one (32 * (out_f * in_f + out_f) floats) they are stored and gemm_finish_kernel adds them.  g_b rides as the row sums
    of the gated dY^T operand, taken by column-block 0 only; when g_W is not asked for it is colsum_kernel, ceil(rows / 512)
    row blocks meeting in atomicAdd, one row block when a workspace pointer is given.  g_X = dY . W is one stored launch.
    The gate keeps dY where gate > 0.
  * the dense distance bank (PN_COMPACT=0) moves from gemm_kernel to gemm3_kernel when ceil(N / 128) * ceil(L * H / 128) >=
    384 (gemm3_pays), and at the same point the fp16 recurrence's operand range is no longer taken in the GEMM epilogues
    (bank_epilogue_range) but by the separate range kernels."""
import itertools

import numpy as np
import pytest
import torch

from gradcheck import assert_grads_close, named_grads
from oracle import pagg_oracle as po

gpu = pytest.mark.gpu
SENT = -77.0
PAD = 67                    # guard floats in front of and behind every operand / output (odd: nothing may rely on alignment)
LD_PAD = 3                  # NaN elements at the end of every leading dimension pn_gemm_f32 is given
UNIT = 2.0 ** -24           # unit roundoff of fp32


def ceil_div(a, b):
    return -(-a // b)


def round32(a):
    return ceil_div(a, 32) * 32


# ------------------------------------------------------------------------------------------------
# the chunking rules, restated
# ------------------------------------------------------------------------------------------------
def fwd_chunks(rows, in_f, out_f):
    """pn_linear_forward with a full workspace -> (first nz, chunks launched, chunk length, length of the last chunk)"""
    tiles = ceil_div(rows, 64) * ceil_div(out_f, 64)
    nz0 = max(1, min(8, ceil_div(512, tiles), in_f // 64))
    if nz0 <= 1:
        return 1, 1, in_f, in_f
    chunk = round32(ceil_div(in_f, nz0))
    nz = ceil_div(in_f, chunk)
    return nz0, nz, chunk, in_f - (nz - 1) * chunk


def bwd_chunks(rows, det):
    """the weight gradient of pn_linear_backward -> (chunks over `rows`, chunk length, length of the last chunk)"""
    ksplit = max(1, ceil_div(rows, 256))
    if det:
        ksplit = min(ksplit, 32)
    chunk = max(32, round32(ceil_div(rows, ksplit)))
    nz = ceil_div(rows, chunk)
    return nz, chunk, rows - (nz - 1) * chunk


def colsum_blocks(rows, workspace):
    """row blocks of colsum_kernel (the g_b-only route)"""
    return 1 if workspace else min(1024, ceil_div(rows, 512))


# ------------------------------------------------------------------------------------------------
# case tables
# ------------------------------------------------------------------------------------------------
EDGES = (1, 31, 33, 63, 64, 65, 129)
GEMM_MN = ((1, 1), (65, 129), (129, 65), (31, 33), (33, 63), (63, 64), (64, 31))
GEMM_K = (1, 31, 32, 33, 64, 95, 96, 97, 127, 128, 129, 160, 161)
GEMM_LAYOUTS = ((True, True), (True, False), (False, True), (False, False))     # (A K-contiguous, B K-contiguous)
GEMM_STREAM_K = (127, 128, 129, 161)            # these K run on a non-default stream: both kernels in the K-contiguous layout
GEMM_EPILOGUES = tuple(itertools.product((False, True), (0, 1), (0, 5)))        # (bias, relu, ldc - N)

FWD_SHAPES = ((65, 127, 65),       # no split although a workspace is passed (K // 64 = 1): gemm_k128_kernel
              (65, 130, 65),       # nz = 2, last chunk 34
              (33, 193, 64),       # nz = 3, last chunk ONE element
              (129, 257, 31),      # first nz 4, chunk 96 -> 3 chunks launched
              (64, 512, 64),       # nz = 8, every chunk full
              (1, 768, 1),         # nz = 8, one output element
              (65, 1433, 65))      # Cora's unaligned in_f: nz = 8, chunk 192, last chunk 89

BWD_ROWS = (1, 255, 256, 257, 511, 512, 513, 1025)
BWD_OUT_F = (1, 63, 64, 65)
BWD_IN_F = (1, 33, 64, 65, 130)


def bwd_shapes(rows):
    """(out_f, in_f) run at this row count: half of the cross product, the other half at the next row count; the two
    corners at every one"""
    r = BWD_ROWS.index(rows)
    s = {(o, i) for a, o in enumerate(BWD_OUT_F) for b, i in enumerate(BWD_IN_F) if (a + b + r) % 2 == 0}
    return sorted(s | {(1, 1), (65, 130)})


def bank_tiles(N, L=6, H=128):
    return ceil_div(N, 128) * ceil_div(L * H, 128)


BANK_N = (8064, 8065)


def test_case_tables_reach_every_route():
    """CPU: the tables above really produce the routes the GPU tests are there for, so a later edit of a table cannot
    hollow the coverage out silently."""
    # pn_gemm_f32: every edge in both positions, the three named pairs, both sides of 128, every epilogue combination
    assert {m for m, _ in GEMM_MN} == set(EDGES) and {n for _, n in GEMM_MN} == set(EDGES)
    assert {(1, 1), (65, 129), (129, 65)} <= set(GEMM_MN)
    assert set(GEMM_K) == {1, 31, 32, 33, 64, 95, 96, 97, 127, 128, 129, 160, 161}
    assert len(set(GEMM_LAYOUTS)) == 4 and len(set(GEMM_EPILOGUES)) == 8
    assert any(k <= 128 for k in GEMM_STREAM_K) and any(k > 128 for k in GEMM_STREAM_K) and set(GEMM_STREAM_K) <= set(GEMM_K)
    assert max(GEMM_K) * 64 < 2 ** 24
    # every ReLU case of 64 results or more holds exact zeros and negatives in front of the ReLU
    for (M, N), K in itertools.product(GEMM_MN, GEMM_K):
        if M * N >= 64:
            A, B, bias = gemm_operands(M, N, K)
            for pre in (A.double() @ B.double().t(), A.double() @ B.double().t() + bias.double()):
                assert (pre == 0).any() and (pre < 0).any() and (pre > 0).any(), (M, N, K)
    # pn_linear_forward
    info = {s: fwd_chunks(*s) for s in FWD_SHAPES}
    assert {v[1] for v in info.values()} >= {1, 2, 3, 8}
    assert info[(65, 127, 65)][1] == 1 and info[(65, 130, 65)][1:] == (2, 96, 34)
    assert any(nz > 1 and tail == 1 for _, nz, _, tail in info.values())
    assert any(nz < nz0 for nz0, nz, _, _ in info.values())
    assert info[(65, 1433, 65)] == (8, 8, 192, 89)
    assert all(in_f * 64 < 2 ** 24 for _, in_f, _ in FWD_SHAPES)
    # pn_linear_backward
    assert {bwd_chunks(r, False)[0] for r in BWD_ROWS} >= {1, 2, 3, 5}
    assert any(bwd_chunks(r, True)[0] >= 2 for r in BWD_ROWS) and any(bwd_chunks(r, True)[0] >= 5 for r in BWD_ROWS)
    assert any(colsum_blocks(r, False) >= 3 for r in BWD_ROWS) and all(colsum_blocks(r, True) == 1 for r in BWD_ROWS)
    seen = set()
    for r in BWD_ROWS:
        seen |= {(r, o, i) for o, i in bwd_shapes(r)}
        assert (65, 130) in bwd_shapes(r) and (1, 1) in bwd_shapes(r)
        assert r * 64 < 2 ** 24
    assert {o for _, o, _ in seen} == set(BWD_OUT_F) and {i for _, _, i in seen} == set(BWD_IN_F)
    assert {(o, i) for _, o, i in seen} == set(itertools.product(BWD_OUT_F, BWD_IN_F))
    assert any(i > 64 for _, _, i in seen)          # more than one column block: the row sums come from block 0 only
    # the gate: every value class in every row and column residue class modulo 64
    g = gate_tensor(320, 65)
    cls = gate_classes(g)
    assert set(cls.flatten().tolist()) == {0, 1, 2, 3, 4}
    rr, cc = np.meshgrid(np.arange(320) % 64, np.arange(65) % 64, indexing="ij")
    for v in range(5):
        assert set(rr[cls == v].tolist()) == set(range(64)) and set(cc[cls == v].tolist()) == set(range(64))
    cls1 = gate_classes(gate_tensor(1025, 1))       # one column: the rows alone carry every class to every residue
    for v in range(5):
        assert set((np.arange(1025) % 64)[cls1[:, 0] == v].tolist()) == set(range(64))
    assert torch.equal(g > 0, torch.as_tensor((cls == 3) | (cls == 4)))
    # the dense bank's dispatch line
    assert bank_tiles(BANK_N[0]) == 378 < 384 == bank_tiles(BANK_N[1]) and BANK_N[1] % 128 == 1


# ------------------------------------------------------------------------------------------------
# operands and guards
# ------------------------------------------------------------------------------------------------
def ints(gen, *shape):
    return torch.randint(-8, 9, shape, generator=gen).float()


def gemm_operands(M, N, K):
    gen = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
    A, B, bias = ints(gen, M, K), ints(gen, N, K), ints(gen, N)
    if M > 1:           # row 0 gives bias[n] (or 0): an exact zero in front of the ReLU in every case
        A[0] = 0.0
        bias[0] = 0.0
    return A, B, bias


def gate_tensor(rows, out_f):
    """0.0, -0.0, a negative integer, a positive integer, the smallest positive normal: class (r + c) % 5"""
    r, c = torch.arange(rows)[:, None], torch.arange(out_f)[None, :]
    k = ((r * 7 + c) % 8 + 1).float()
    tiny = torch.finfo(torch.float32).tiny
    vals = torch.stack([torch.zeros(rows, out_f), torch.full((rows, out_f), -0.0), -k, k, torch.full((rows, out_f), tiny)])
    return vals.gather(0, ((r + c) % 5)[None])[0].contiguous()


def gate_classes(g):
    a = g.numpy()
    tiny = np.float32(torch.finfo(torch.float32).tiny)
    return np.where(a == tiny, 4, np.where(a > 0, 3, np.where(a < 0, 2, np.where(np.signbit(a), 1, 0))))


class Guarded:
    """a device tensor of `shape` (row pitch ld >= shape[-1]) inside a larger allocation filled with `fill`"""

    def __init__(self, shape, fill, ld=None, values=None):
        shape = tuple(shape)
        rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
        self.cols = shape[-1]
        self.ld = self.cols if ld is None else ld
        self.rows, self.fill = rows, fill
        self.buf = torch.full((PAD + rows * self.ld + PAD,), fill, dtype=torch.float32, device="cuda")
        self.win = self.buf[PAD:PAD + rows * self.ld].view(rows, self.ld)
        if values is not None:
            self.win[:, :self.cols].copy_(values.reshape(rows, self.cols))

    def ptr(self):
        return self.win.data_ptr()

    def host(self):
        """a copy on the CPU, after everything queued on the device: one transfer for all the checks of a launch"""
        h = Guarded.__new__(Guarded)
        h.cols, h.ld, h.rows, h.fill = self.cols, self.ld, self.rows, self.fill
        h.buf = self.buf.cpu()
        h.win = h.buf[PAD:PAD + h.rows * h.ld].view(h.rows, h.ld)
        return h

    def values(self):
        return self.win[:, :self.cols]

    def untouched_outside(self):
        """pad columns, the floats in front and behind"""
        return bool((self.buf[:PAD] == self.fill).all() and (self.buf[PAD + self.rows * self.ld:] == self.fill).all() and
                    (self.win[:, self.cols:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


def operand(t, ld_pad=0):
    """t on the device, NaN around it (and in ld_pad elements behind every row)"""
    t = t.contiguous()
    return Guarded(t.shape if t.dim() > 1 else (1, t.numel()), float("nan"), ld=t.shape[-1] + ld_pad, values=t)


def output(rows, cols, ld=None):
    return Guarded((rows, cols), SENT, ld=ld)


def rounding_bound(absA, absB, absbias, K, nz):
    """|C - C64| <= (K + nz + 2) u (|A| |B|^T + |bias|), u = 2^-24: the forward bound of a length-K fp32 dot product in any
    summation order (K products, K - 1 additions, the bias), with nz further additions for the chunk finish"""
    rhs = absA.double() @ absB.double().t()
    if absbias is not None:
        rhs = rhs + absbias.double()
    return (K + nz + 2) * UNIT * rhs


def assert_within(got, want64, bound, what):
    err = (got.double().cpu() - want64).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print("%s: max |err| / bound = %.3g" % (what, worst))
    assert torch.isfinite(got).all() and bool((err <= bound).all()), (what, worst)


# ------------------------------------------------------------------------------------------------
# part A: pn_gemm_f32
# ------------------------------------------------------------------------------------------------
def place_gemm_operand(T, k_contig):
    """T [R, K] as pn_gemm_f32 reads it -> (guarded storage, stride of the row index, stride of k)"""
    R, K = T.shape
    if k_contig:
        return operand(T, LD_PAD), K + LD_PAD, 1
    return operand(T.t(), LD_PAD), 1, R + LD_PAD


def place_gemm(A, B, bias, a_kc, b_kc):
    return place_gemm_operand(A, a_kc) + place_gemm_operand(B, b_kc) + (operand(bias),)


def run_gemm(lib, _lib, placed, M, N, K, use_bias, relu, ldc_pad, stream=None):
    """-> the guarded output, copied to the host"""
    assert K * 64 < 2 ** 24
    ga, sAm, sAk, gb, sBn, sBk, gbias = placed
    C = output(M, N, N + ldc_pad)
    if stream is not None:
        torch.cuda.synchronize()            # the operands were written on the current stream
    _lib.check(lib.pn_gemm_f32(ga.ptr(), sAm, sAk, gb.ptr(), sBn, sBk, C.ptr(), N + ldc_pad, gbias.ptr() if use_bias else None,
                               M, N, K, relu, stream.cuda_stream if stream is not None else None))
    if stream is not None:
        stream.synchronize()
    return C.host()


@gpu
@pytest.mark.parametrize("a_kc,b_kc", GEMM_LAYOUTS)
def test_gemm_f32_is_exact_at_tile_and_k_edges(a_kc, b_kc):
    """All four operand layouts x the M / N edges x K on both sides of every K tile and of 128 x bias x ReLU x ldc:
    bit-equal to the fp64 product of the integer operands, nothing outside the window written, no NaN guard read."""
    from pathnet_amd import _lib
    lib = _lib.load()
    side = torch.cuda.Stream()
    for (M, N), K in itertools.product(GEMM_MN, GEMM_K):
        A, B, bias = gemm_operands(M, N, K)
        pre = A.double() @ B.double().t()
        placed = place_gemm(A, B, bias, a_kc, b_kc)
        for use_bias, relu, ldc_pad in GEMM_EPILOGUES:
            want = pre + bias.double() if use_bias else pre
            want = (torch.relu(want) if relu else want).float()
            stream = side if K in GEMM_STREAM_K and (use_bias, relu, ldc_pad) in ((True, 1, 5), (False, 0, 0)) else None
            C = run_gemm(lib, _lib, placed, M, N, K, use_bias, relu, ldc_pad, stream)
            case = (M, N, K, use_bias, relu, ldc_pad, stream is not None)
            assert torch.equal(C.values(), want), case
            assert C.untouched_outside(), case


@gpu
def test_gemm_f32_empty_and_bad_arguments():
    """M == 0 or N == 0: OK, C untouched.  K == 0 and strides with neither equal to 1: an error, C untouched."""
    from pathnet_amd import _lib
    lib = _lib.load()
    A, B, bias = gemm_operands(5, 7, 9)
    ga, gb, gbias = operand(A), operand(B), operand(bias)
    C = output(5, 7)

    def call(M, N, K, sAm=9, sAk=1, sBn=9, sBk=1):
        return lib.pn_gemm_f32(ga.ptr(), sAm, sAk, gb.ptr(), sBn, sBk, C.ptr(), 7, gbias.ptr(), M, N, K, 0, None)
    assert call(0, 7, 9) == _lib.PN_OK and call(5, 0, 9) == _lib.PN_OK and call(0, 0, 0) == _lib.PN_OK
    assert call(5, 7, 0) != _lib.PN_OK
    with pytest.raises(_lib.PnError):
        _lib.check(call(5, 7, 0))
    assert call(5, 7, 3, sAm=3, sAk=2) != _lib.PN_OK
    assert call(5, 7, 3, sBn=3, sBk=2) != _lib.PN_OK
    with pytest.raises(_lib.PnError):
        _lib.check(call(5, 7, 3, sAm=2, sAk=2, sBn=2, sBk=2))
    assert C.host().untouched()
    _lib.check(call(5, 7, 9))           # the arguments were good ones
    assert torch.equal(C.host().values(), (A.double() @ B.double().t() + bias.double()).float())


@gpu
@pytest.mark.parametrize("K", [97, 161])
def test_gemm_f32_rounds_like_fp32(K):
    """randn operands, both kernels (K on either side of 128): within the componentwise bound of an fp32 dot product"""
    from pathnet_amd import _lib
    lib = _lib.load()
    gen = torch.Generator().manual_seed(K)
    M, N = 65, 129
    A, B, bias = torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen), torch.randn(N, generator=gen)
    want = A.double() @ B.double().t() + bias.double()
    for a_kc, b_kc in GEMM_LAYOUTS:
        C = run_gemm(lib, _lib, place_gemm(A, B, bias, a_kc, b_kc), M, N, K, True, 0, 5)
        assert_within(C.values(), want, rounding_bound(A.abs(), B.abs(), bias.abs(), K, 0), ("gemm", K, a_kc, b_kc))
        assert C.untouched_outside()


# ------------------------------------------------------------------------------------------------
# part B: pn_linear_forward / pn_linear_backward
# ------------------------------------------------------------------------------------------------
def linear_forward(lib, _lib, X, W, b, rows, in_f, out_f, relu, ws_floats=None, ws_bytes=None):
    """-> (Y, workspace): both guarded and copied to the host, the workspace sentinel-filled"""
    gx, gw, gb = operand(X), operand(W), operand(b)
    Y = output(X.shape[0], out_f)           # (room for every row of X, also when the call is told of fewer)
    ws = output(1, ws_floats) if ws_floats else None
    _lib.check(lib.pn_linear_forward(_lib.context("cuda"), gx.ptr(), gw.ptr(), gb.ptr(), rows, in_f, out_f, relu, Y.ptr(),
                                     ws.ptr() if ws else None, ws_bytes if ws else 0, None))
    return Y.host(), ws.host() if ws else None


@gpu
@pytest.mark.parametrize("rows,in_f,out_f", FWD_SHAPES)
def test_linear_forward_is_exact_on_every_split_route(rows, in_f, out_f):
    """No workspace, a full workspace (PN_LINEAR_SPLIT_MAX * rows * out_f floats) and one a byte too small, which must
    fall back without touching it: all bit-equal to the integer reference, with and without ReLU."""
    from pathnet_amd import _lib
    lib = _lib.load()
    assert in_f * 64 < 2 ** 24
    gen = torch.Generator().manual_seed(7919 * rows + 31 * in_f + out_f)
    X, W, b = ints(gen, rows, in_f), ints(gen, out_f, in_f), ints(gen, out_f)
    if rows > 1:
        X[0] = 0.0
        b[0] = 0.0
    pre = X.double() @ W.double().t() + b.double()
    full = _lib.LINEAR_SPLIT_MAX * rows * out_f
    nz = fwd_chunks(rows, in_f, out_f)[1]
    for relu in (0, 1):
        want = (torch.relu(pre) if relu else pre).float()
        for name, ws_bytes in (("none", None), ("full", 4 * full), ("short", 4 * full - 1)):
            Y, ws = linear_forward(lib, _lib, X, W, b, rows, in_f, out_f, relu, full if ws_bytes else None, ws_bytes)
            assert torch.equal(Y.values(), want), (name, relu)
            assert Y.untouched_outside(), (name, relu)
            if name == "short":
                assert ws.untouched(), "a workspace that is too small was written"
            elif name == "full":
                assert ws.untouched_outside()
                used = int((ws.values() != SENT).sum().item())          # (a chunk sum of exactly -77 would hide one float)
                assert used <= nz * rows * out_f if nz > 1 else used == 0, (used, nz)
    # rows == 0: nothing happens (the pointers are good ones)
    Y, ws = linear_forward(lib, _lib, X, W, b, 0, in_f, out_f, 1, full, 4 * full)
    assert Y.untouched() and ws.untouched()


@gpu
def test_linear_forward_rounds_like_fp32():
    """randn operands at Cora's in_f, eight chunks: within the fp32 bound with the finish's eight further additions"""
    from pathnet_amd import _lib
    lib = _lib.load()
    rows, in_f, out_f = 65, 1433, 65
    gen = torch.Generator().manual_seed(5)
    X, W, b = torch.randn(rows, in_f, generator=gen), torch.randn(out_f, in_f, generator=gen), torch.randn(out_f, generator=gen)
    want = X.double() @ W.double().t() + b.double()
    full = _lib.LINEAR_SPLIT_MAX * rows * out_f
    nz = fwd_chunks(rows, in_f, out_f)[1]
    assert nz == 8
    for ws_bytes, extra in ((None, 0), (4 * full, nz)):
        Y, _ = linear_forward(lib, _lib, X, W, b, rows, in_f, out_f, 0, full if ws_bytes else None, ws_bytes)
        assert_within(Y.values(), want, rounding_bound(X.abs(), W.abs(), b.abs(), in_f, extra), ("linear_forward", extra))


class BackwardCase:
    """operands of one pn_linear_backward case on the device (NaN around each), and the expected outputs"""

    def __init__(self, rows, in_f, out_f, gated, integer=True):
        self.rows, self.in_f, self.out_f = rows, in_f, out_f
        gen = torch.Generator().manual_seed(104729 * rows + 613 * in_f + 7 * out_f + int(gated))
        r = max(rows, 1)        # (rows == 0: the pointers must still be good ones)
        draw = (lambda *s: ints(gen, *s)) if integer else (lambda *s: torch.randn(*s, generator=gen))
        self.dY, self.X, self.W = draw(r, out_f), draw(r, in_f), draw(out_f, in_f)
        self.gate = gate_tensor(r, out_f) if gated else None
        self.g_dY, self.g_X, self.g_W = operand(self.dY), operand(self.X), operand(self.W)
        self.g_gate = operand(self.gate) if gated else None
        d = self.dY[:rows].double()
        if gated:
            d = d * (self.gate[:rows] > 0)
        self.d = d
        self.want = {"W": d.t() @ self.X[:rows].double(), "b": d.sum(0), "X": d @ self.W.double()}

    def run(self, lib, _lib, outs, workspace):
        """outs: subset of "WbX".  workspace: None, or True for PN_LINEAR_BWD_SPLIT_MAX * (out_f * in_f + out_f) floats.
        -> {name: guarded output}, the guarded workspace, copied to the host"""
        o = {"W": output(self.out_f, self.in_f), "b": output(1, self.out_f), "X": output(max(self.rows, 1), self.in_f)}
        ws = output(1, _lib.LINEAR_BWD_SPLIT_MAX * (self.out_f * self.in_f + self.out_f)) if workspace else None
        p = {k: (o[k].ptr() if k in outs else None) for k in o}
        _lib.check(lib.pn_linear_backward(_lib.context("cuda"), self.g_dY.ptr(), self.g_gate.ptr() if self.g_gate else None,
                                          self.g_X.ptr(), self.g_W.ptr(), self.rows, self.in_f, self.out_f, p["W"], p["b"], p["X"],
                                          ws.ptr() if ws else None, 4 * ws.cols if ws else 0, None))
        return {k: v.host() for k, v in o.items()}, ws.host() if ws else None

    def check_exact(self, o, outs, tag):
        for k in "WbX":
            if k not in outs:
                assert o[k].untouched(), (tag, k, "an output that was not asked for was written")
                continue
            got = o[k].values()
            if k == "X":
                got = got[:self.rows]
            assert torch.equal(got.reshape(self.want[k].shape), self.want[k].float()), (tag, k)
            assert o[k].untouched_outside(), (tag, k)


BWD_SUBSETS = ("WbX", "W", "b", "X")


@gpu
@pytest.mark.parametrize("rows", BWD_ROWS)
def test_linear_backward_is_exact_on_every_route(rows):
    """The atomic route, the workspace route (twice: bit-equal to each other too) and the g_b-only route with and
    without a workspace; every output subset; no gate, and a gate holding 0.0, -0.0, negative and positive integers and
    the smallest positive normal (expected mask: gate > 0, the same for g_W, g_b and g_X).  The windows of g_W / g_b start
    out as the sentinel: the call zero-fills and overwrites."""
    from pathnet_amd import _lib
    lib = _lib.load()
    assert rows * 64 < 2 ** 24 and max(BWD_OUT_F) * 64 < 2 ** 24
    for (out_f, in_f), gated in itertools.product(bwd_shapes(rows), (False, True)):
        c = BackwardCase(rows, in_f, out_f, gated)
        for workspace, outs in itertools.product((None, True), BWD_SUBSETS):
            tag = (rows, in_f, out_f, gated, bool(workspace), outs)
            o, ws = c.run(lib, _lib, outs, workspace)
            c.check_exact(o, outs, tag)
            if ws:
                assert ws.untouched_outside(), tag
            if workspace and outs == "WbX":
                o2, _ = c.run(lib, _lib, outs, workspace)
                c.check_exact(o2, outs, tag)
                for k in outs:
                    assert torch.equal(o[k].buf, o2[k].buf), (tag, k)


@gpu
@pytest.mark.parametrize("gated", [False, True])
def test_linear_backward_without_rows_zeroes_the_parameter_gradients(gated):
    """rows == 0: g_W and g_b are zero (not left as they were), g_X -- zero rows -- is not touched"""
    from pathnet_amd import _lib
    lib = _lib.load()
    c = BackwardCase(0, 33, 65, gated)
    for workspace in (None, True):
        o, ws = c.run(lib, _lib, "WbX", workspace)
        assert bool((o["W"].values() == 0).all()) and bool((o["b"].values() == 0).all())
        assert o["W"].untouched_outside() and o["b"].untouched_outside() and o["X"].untouched()
        assert ws is None or ws.untouched()


@gpu
def test_linear_backward_rounds_like_fp32():
    """randn operands, gated, five chunks over the rows: g_W and g_b within the fp32 bound of a length-`rows` reduction
    with the chunks' further additions (atomic or finish), g_X within that of a length-out_f one"""
    from pathnet_amd import _lib
    lib = _lib.load()
    rows, in_f, out_f = 1025, 130, 65
    c = BackwardCase(rows, in_f, out_f, True, integer=False)
    nz = bwd_chunks(rows, True)[0]
    assert nz == 5 == bwd_chunks(rows, False)[0]
    ones = torch.ones(1, rows)
    bounds = {"W": rounding_bound(c.d.abs().t(), c.X.abs().t(), None, rows, nz),
              "b": rounding_bound(c.d.abs().t(), ones, None, rows, nz)[:, 0],
              "X": rounding_bound(c.d.abs(), c.W.abs().t(), None, out_f, 0)}
    for workspace in (None, True):
        o, _ = c.run(lib, _lib, "WbX", workspace)
        for k in "WbX":
            assert_within(o[k].values().reshape(c.want[k].shape), c.want[k], bounds[k], ("linear_backward", k, bool(workspace)))
    for workspace in (None, True):          # g_b alone: colsum_kernel, three row blocks or one
        o, _ = c.run(lib, _lib, "b", workspace)
        assert_within(o["b"].values().reshape(-1), c.want["b"], rounding_bound(c.d.abs().t(), ones, None, rows, colsum_blocks(
            rows, workspace))[:, 0], ("linear_backward colsum", bool(workspace)))


# ------------------------------------------------------------------------------------------------
# part C: the dense bank's dispatch line, through the aggregator
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("variant", ["homo", "hetero"])
def test_dense_bank_on_both_sides_of_the_gemm3_line_matches_the_oracle(variant, monkeypatch):
    """PN_COMPACT=0, L = 6, H = 128: at N = 8064 the bank is 63 x 6 = 378 tiles of 128 x 128 and stays on gemm_kernel (fc0
    and the bank take the fp16 recurrence's operand range in their epilogues); at N = 8065 it is 64 x 6 = 384 tiles, runs
    on gemm3_kernel with one row in its last row tile, and the range comes from the separate kernels.  pn_pagg_shape_info
    reports the dense bank and the arithmetic, not the GEMM kernel: that follows from the tile arithmetic above
    (gemm3_pays, restated in bank_tiles and held by the CPU test).  Node N - 1 is forced into several paths at several
    codes; logits and every gradient, X included, against the CPU oracle; and the two N agree with each other on paths
    that avoid node 8064."""
    import pathnet_amd
    from pathnet_amd import _lib, modules
    from test_gpu_batching import no_relu_ties
    from test_gpu_pagg import run_module, zero_ok
    monkeypatch.setenv("PN_COMPACT", "0")
    F, H, C, W, L, S = 32, 128, 5, 8, 6, 60
    rng = np.random.default_rng(93)
    Nmax = max(BANK_N)
    torch.manual_seed(93)
    X_all = torch.rand(Nmax, F)
    G = torch.randn(S, C)
    sel = np.sort(rng.permutation(min(BANK_N) - 1)[:S])
    base_ids = rng.integers(0, min(BANK_N), (S, W, L))           # no node 8064
    base_ids[:, :, 0] = sel[:, None]
    codes = np.minimum(rng.integers(0, L, (S, W, L)), np.arange(L)[None, None, :])
    plain = {}
    for N in BANK_N:
        torch.manual_seed(94)           # the same parameters for both N
        cls = {"hetero": pathnet_amd.PathNet, "homo": pathnet_amd.PathNet_homo}[variant]
        m = cls(F, H, C, L).cuda().eval()
        if variant == "homo":
            no_relu_ties(m)
        X = X_all[:N].clone()
        mask = np.zeros(N, bool)
        mask[sel] = True
        with torch.no_grad():
            plain[N] = run_module(m, X.cuda(), base_ids, codes, mask, W, L).cpu()
        info = modules.shape_info(m._last_shape[0])
        assert info[0] is False and info[3] == _lib.SEQ_MATH_F16X2, info       # dense bank, the fp16 recurrence
        ids, cds = base_ids.copy(), codes.copy()
        for j in range(12):             # node N - 1 at every step but the first, at codes 0 .. 5
            s, w, t = (5 * j + 1) % S, j % W, 1 + j % (L - 1)
            ids[s, w, t], cds[s, w, t] = N - 1, min(j % L, t)
        node, code, *_ = po.plan(variant, ids, cds, S, W, L)
        assert len(set(code[node == N - 1].tolist())) >= 3
        Xd = X.cuda().requires_grad_(True)
        out = run_module(m, Xd, ids, cds, mask, W, L)
        out.backward(G.cuda())
        pr = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
        Xr = X.clone().requires_grad_(True)
        want = po.forward(variant, pr, Xr, ids, cds, sel, W, L)
        err = (out.detach().cpu() - want.detach()).abs().max().item()
        print("N = %d: logits off by %.3g" % (N, err))
        assert err < 1e-5, (N, err)
        want.backward(G)
        ref = {k: pr[k].grad for k, _ in m.named_parameters()}
        ref["X"] = Xr.grad
        assert Xr.grad[N - 1].abs().max().item() > 0
        assert_grads_close(named_grads(m, {"X": Xd.grad}), ref, zero_ok=zero_ok(variant))
        want_plain = po.forward(variant, {k: v.detach().cpu() for k, v in m.state_dict().items()}, X, base_ids, codes, sel, W, L)
        assert (plain[N] - want_plain).abs().max().item() < 1e-5, N
    across = (plain[BANK_N[0]] - plain[BANK_N[1]]).abs().max().item()
    print("the two routes differ by %.3g" % across)
    assert across < 1e-5, across
