// pn_gemm.h -- the dense GEMM launchers of the aggregator's node-level layers (pn_gemm.hip).  Not part of the ABI.
// A launch is described by one parameter struct (GemmParams / Gemm3Params: what the kernel receives), made by one of the three
// builders below -- linear forward, weight gradient, input gradient -- and then adjusted field by field at the call site.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "pn_internal.h"

namespace pn {

// ---- gemm_kernel: C[m][n] (op)= act( sum_k A(m,k) * B(n,k) + bias[n] ) on the fp32-input MFMA, 64 x 64 tiles ------------------
//   A(m,k) = A[m*sAm + k*sAk] (optionally multiplied by [gateA(m,k) > 0]), B(n,k) = B[n*sBn + k*sBk]; exactly one stride of
//   each operand is 1.
constexpr int GEMM_BM = 64, GEMM_BN = 64, GEMM_KT = 32;
enum { GEMM_STORE = 0, GEMM_ADD = 1, GEMM_ATOMIC = 2, GEMM_PARTIAL = 3 };   // PARTIAL: raw sums of K chunk z to C[z][M][ldc]
// row lists (GemmParams::seg / list; b = seg[0]):
enum { GEMM_IND_NONE = 0,
       GEMM_IND_A_ROWS = 1,     // A row m = list[b + m] (rows of Xh by node), C row m = b + m (compact rows)
       GEMM_IND_C_ROWS = 2,     // A row m = b + m (compact rows), C row m = list[b + m]
       GEMM_IND_K = 3 };        // reduction index k: A column k = b + k (compact rows), B column k = list[b + k]

struct GemmParams {
    const float *A;
    int64_t sAm, sAk;
    const float *gateA;
    const float *B;
    int64_t sBn, sBk;
    float *C;
    int64_t ldc;
    const float *bias;
    int M, N, K;
    int relu, mode;
    int kchunk;  // K range per blockIdx.z (launch_gemm derives it from its ksplit, on its own copy)
    float *rowsum;  // optional [M]: += sum_k A(m,k) (after gating) -- the bias gradient that goes with a dW GEMM
                    // (PARTIAL: [nz][M], chunk z stores its own sums)
    // Compact rows (the distance bank over the (node, code) rows a batch touches, GEMM_IND_*): `list` holds the node of every
    // compact row, the launch covers rows [seg[0], seg[1]) of it -- counts that exist in device memory only; M (or K) given
    // on the host is their upper bound (it sizes the grid), workgroups past the real count leave at once.
    const int32_t *seg, *list;
    int ind;
    // operand range of the fp16 recurrence taken where the values are produced (run_tables; SeqRange of pn_seq.h, whose first
    // three words these point to): absmax[0] = atomicMax of the bit patterns of |C| over what this launch stores (after bias /
    // ReLU); absmax[1] += the biased exponents, absmax[2] += the count of the non-zero 32 x 32 sub-tile maxima of every eighth
    // workgroup (the spread statistic); clear_word[0..2] are set to 0 by one thread of the launch -- the GEMM in front of the
    // one that takes the maximum, on the same stream
    uint32_t *absmax, *clear_word;
};

// The three operand layouts of a linear layer Y = X . W^T (X [rows, in_f], W [out_f, in_f], Y / dY [rows, out_f]; every matrix
// row-major with its leading dimension).  Each returns the plain launch: no gate, no bias, no ReLU, GEMM_STORE, no row sums, no
// row list, no range words.
// forward:          Y[rows, out_f] = X . W^T                     (both operands contiguous along the reduction, in_f)
inline GemmParams gemm_linear_fwd(const float *X, int64_t ldx, const float *W, int64_t ldw, float *Y, int64_t ldy, int rows,
                                  int in_f, int out_f) {
    GemmParams g{};
    g.A = X, g.sAm = ldx, g.sAk = 1;
    g.B = W, g.sBn = ldw, g.sBk = 1;
    g.C = Y, g.ldc = ldy;
    g.M = rows, g.N = out_f, g.K = in_f;
    return g;
}
// weight gradient:  g_W[out_f, in_f] = dY^T . X                  (the reduction runs over the rows; callers accumulate: mode)
inline GemmParams gemm_weight_grad(const float *dY, int64_t lddy, const float *X, int64_t ldx, float *g_W, int64_t ldgw, int rows,
                                   int in_f, int out_f) {
    GemmParams g{};
    g.A = dY, g.sAm = 1, g.sAk = lddy;
    g.B = X, g.sBn = 1, g.sBk = ldx;
    g.C = g_W, g.ldc = ldgw;
    g.M = out_f, g.N = in_f, g.K = rows;
    return g;
}
// input gradient:   g_X[rows, in_f] = dY . W                     (the reduction runs over out_f: W is read by columns)
inline GemmParams gemm_input_grad(const float *dY, int64_t lddy, const float *W, int64_t ldw, float *g_X, int64_t ldgx, int rows,
                                  int in_f, int out_f) {
    GemmParams g{};
    g.A = dY, g.sAm = lddy, g.sAk = 1;
    g.B = W, g.sBn = 1, g.sBk = ldw;
    g.C = g_X, g.ldc = ldgx;
    g.M = rows, g.N = in_f, g.K = out_f;
    return g;
}

// ksplit > 1 (ATOMIC / PARTIAL modes): the reduction is cut into that many chunks over blockIdx.z.
int launch_gemm(hipStream_t stream, const GemmParams &g, int ksplit = 1);
// K chunks a split node-level GEMM is cut into (1 = not split): aim at ~2 workgroups per CU, at least two K tiles each
constexpr int GEMM_MAX_SPLIT = 8;
int gemm_split_count(int M, int N, int K);
// STORE / ADD GEMM with the reduction split over gemm_split_count chunks: chunk sums to `partial` ([nz][M][N]), then one fixed-order
// finish launch (bias / ReLU / accumulate).  partial == nullptr: one launch_gemm
int launch_gemm_split(hipStream_t stream, const GemmParams &g, float *partial);
// deterministic weight-gradient GEMM: C += A . B^T and rowsum += row sums of A, chunk sums stored and added in chunk order
// (g.mode is not read: the same description serves launch_gemm's GEMM_ATOMIC route)
constexpr int DET_MAX_SPLIT = 32;
inline size_t det_gemm_floats(size_t M, size_t N) { return (size_t)DET_MAX_SPLIT * (M * N + M); }
int launch_gemm_det(hipStream_t stream, const GemmParams &g, int ksplit, float *partial);
// out[n] (+)= sum_m A[m*ld + n] * [gate[m*ld+n] > 0]  (bias gradients); det: one workgroup per 64 columns, a single add per output
int launch_colsum(hipStream_t stream, const float *A, const float *gate, int64_t ld, int M, int N, float *out, bool det = false);
int launch_transpose(hipStream_t stream, const float *in, int R, int C, float *out);      // out [C, R] = in [R, C]^T

// ---- gemm3_kernel: C[m][n] = sum_k A[m*lda + k] * B[n*ldb + k] (+ bias[n]) with fp32 results from the bf16 matrix pipe (three
//      planes, six MFMAs per product), 128 x 128 tiles; both operands K-contiguous, K a multiple of 32 ------------------------------
constexpr int G3_BM = 128, G3_BN = 128, G3_KT = 32;
struct Gemm3Params {
    const float *A;
    int64_t lda;
    const float *B;
    int64_t ldb;
    float *C;
    int64_t ldc;
    const float *bias;
    int M, N, K;
    // node-level GEMMs over a row list (the compact distance bank's forward, GEMM_IND_A_ROWS as in gemm_kernel: the
    // row count lives in device memory, M bounds it), a ReLU gate on A (element kept where gate > 0, same indexing as A),
    // ReLU on the result, C += instead of C =
    const float *gate;
    const int32_t *seg, *list;
    int relu, add;
};
// the same launch from a linear-forward description (gemm_linear_fwd: both operands K-contiguous), GEMM_STORE or GEMM_ADD; the
// kernel has no row sums and no range words, and takes the row-list kind (g.ind: none or GEMM_IND_A_ROWS) as launch_gemm3's argument
inline Gemm3Params gemm3_of(const GemmParams &g) {
    Gemm3Params p{};
    p.A = g.A, p.lda = g.sAm;
    p.B = g.B, p.ldb = g.sBn;
    p.C = g.C, p.ldc = g.ldc;
    p.bias = g.bias;
    p.M = g.M, p.N = g.N, p.K = g.K;
    p.gate = g.gateA;
    p.seg = g.seg, p.list = g.list;
    p.relu = g.relu, p.add = g.mode == GEMM_ADD;
    return p;
}
int launch_gemm3(hipStream_t stream, const Gemm3Params &p, int ind = GEMM_IND_NONE);
// the bf16 x 3 GEMM pays once its 128 x 128 tiles fill the GPU; `which`: bit of the context knob PN_NODE_GEMM3 (a mask of these three)
enum { G3_FC0 = 1, G3_BANK = 2, G3_BANK_DX = 4 };
bool gemm3_pays(const pn_context *ctx, int64_t M, int64_t N, int K, int which);

}  // namespace pn
