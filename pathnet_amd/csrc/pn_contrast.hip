// pn_contrast.hip -- NT-Xent / InfoNCE between two views of the same S nodes, forward and backward, tiled and flash-style:
// no S x S array is ever in memory (include/pathnet_hip.h carries the contract).
//
// The mathematics.  A, B fp32 [S, D]; tau > 0; valid uint8 [S] or NULL; intra 0 / 1.  Pair i is LIVE when valid[i] != 0 (or
// valid is NULL), every entry of a_i and b_i is finite and both norms, formed in fp64, are finite and > 0; M = live pairs, bad
// = pairs that are not live for the data's sake alone.  The unit rows stack as z_r = a_r / |a_r| (r < S), b_{r-S} / |b_{r-S}|
// (r >= S), n = 2S of them; partner p(r) = r +- S; logit s_rc = <z_r, z_c> / tau; N(r) = every live c != r, with intra == 0
// only those of the other view.
//     lse_r = log sum_{c in N(r)} exp(s_rc)       row_loss_r = lse_r - s_{r,p(r)}  (0 for a row that is not live)
//     loss  = (1 / 2M) sum_{live r} row_loss_r    (0 when M == 0)
//     hit_r = s_{r,p(r)} >= s_rc for every c in N(r), on the fp32 logits of the kernel
// Backward, with g the upstream gradient (device) and P_rc = exp(s_rc - lse_r):
//     dz_r = g / (2 M tau) [ sum_{c in N(r)} (P_rc + P_cr) z_c - 2 z_{p(r)} ]
//     dx_r = (dz_r - z_r <z_r, dz_r>) / |x_r|      (exactly 0 for a row that is not live, and when M == 0)
// s is symmetric -- bit for bit: both orders run the same k-ordered fma chain -- so row tile r gets P_rc and P_cr in one pass
// over its column tiles from the saved lse vector; the -2 z_p term rides in the same matrix, W_rc = P_rc + P_cr - 2 [c == p(r)].
//
//   prep_kernel       a wave per pair: fp64 norms, liveness, z = (float)((double)x / norm) (zeros for a pair that is not live)
//   forward_kernel    a workgroup of 256 owns a row tile of 64 and walks the column tiles of 128 in ascending order; per tile
//                     s = Z_r Z_c^T over K chunks of 16 on v_mfma_f32_32x32x2_f32 (exact fp32 products, one fma chain per
//                     element), then every lane folds its two logits of a row into that row's (max, sum) pair: an online
//                     softmax per lane.  At the end the 32 lanes of a row meet in a fixed butterfly, the two column halves in
//                     ascending order; lse = m + log(sum) in fp64.
//   loss_partial / loss_final   row_loss in partials of 256 rows (halving tree, absent slots 0.0), the partials in ascending
//                     order, fp64.  M, bad and hits are integer atomics: exact, order-free.
//   backward_kernel   grid (row tiles, D chunks of 256): recomputes s per column tile, writes W to LDS and multiplies W [64, 128]
//                     by Z_c [128, 256] on the same MFMA into 64 accumulators per lane; stores G = W Z (unscaled) with plain stores
//   finish_kernel     a wave per row, fp64: dx = coef (G - z <z, G>) / norm, coef = g / (2 M tau) read on the device
//
// Every sum's order depends on (S, D, intra) alone.  No floating-point atomic; plain C++ and vector stores only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pn_internal.h"
#include "pn_simtile.h"

namespace {

constexpr int kDC = 256;                 // D chunk of a backward workgroup: 64 columns of G per wave
constexpr int kPart = 256;               // rows per partial of the loss sum
constexpr int kMaxD = 8192;
constexpr double kDblMax = 1.7976931348623157e308;

struct Header {            // the first 64 bytes of the workspace
    unsigned long long M, bad, hits;
    unsigned long long pad[5];
};

struct Ws {
    Header *head;
    double *norm;          // [n]
    double *row_loss;      // [n]
    double *part;          // [ceil(n / 256)]
    float *Z;              // [n, D] unit rows, zeros for a row that is not live
    float *G;              // [n, D] backward: sum_c W_rc z_c
    float *lse;            // [n]
    int32_t *live;         // [n]
};

__host__ __device__ inline int64_t parts_of(int64_t n) { return (n + kPart - 1) / kPart; }

__host__ __device__ inline Ws ws_of(void *base, int64_t S, int32_t D) {
    Ws w;
    const int64_t n = 2 * S;
    char *p = (char *)base;
    w.head = (Header *)p;
    p += sizeof(Header);
    w.norm = (double *)p;
    p += 8 * n;
    w.row_loss = (double *)p;
    p += 8 * n;
    w.part = (double *)p;
    p += 8 * parts_of(n);
    w.Z = (float *)p;
    p += 4 * n * D;
    w.G = (float *)p;
    p += 4 * n * D;
    w.lse = (float *)p;
    p += 4 * n;
    w.live = (int32_t *)p;
    return w;
}

inline int64_t ws_bytes(int64_t S, int32_t D) {
    const int64_t n = 2 * S;
    return (int64_t)sizeof(Header) + 16 * n + 8 * parts_of(n) + 8 * n * D + 8 * n;
}

__device__ inline double wave_sum(double v) {       // a fixed butterfly: the same value, bit for bit, in all 64 lanes
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ inline bool finite_f(float v) { return fabsf(v) <= 3.4028234663852886e38f; }

// ---- prep ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void prep_kernel(const float *__restrict__ A, int64_t lda, const float *__restrict__ B,
                                                        int64_t ldb, int64_t S, int32_t D, const uint8_t *__restrict__ valid,
                                                        void *ws) {
    const Ws w = ws_of(ws, S, D);
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (i >= S) return;
    const float *x[2] = {A + i * lda, B + i * ldb};
    double nrm[2];
    bool ok = true;
    for (int v = 0; v < 2; v++) {
        double ss = 0.0;
        int fin = 1;
        for (int32_t d = lane; d < D; d += 64) {
            const float e = x[v][d];
            if (!finite_f(e)) fin = 0;
            ss += (double)e * (double)e;
        }
        fin = __all(fin);
        ss = wave_sum(fin ? ss : 0.0);
        nrm[v] = sqrt(ss);
        ok = ok && fin && nrm[v] > 0.0 && nrm[v] <= kDblMax;
    }
    const bool wanted = !valid || valid[i] != 0;
    const bool live = wanted && ok;
    for (int v = 0; v < 2; v++) {
        const int64_t r = i + v * S;
        float *z = w.Z + r * D;
        for (int32_t d = lane; d < D; d += 64) z[d] = live ? (float)((double)x[v][d] / nrm[v]) : 0.0f;
        if (lane == 0) {
            w.norm[r] = live ? nrm[v] : 1.0;
            w.live[r] = live ? 1 : 0;
        }
    }
    if (lane == 0) {
        if (live) atomicAdd(&w.head->M, 1ULL);
        else if (wanted) atomicAdd(&w.head->bad, 1ULL);
    }
}

// with intra == 0 a column tile that lies, like the whole row tile, inside one view holds no member of any N(r)
__device__ inline bool tile_skipped(int64_t r0, int64_t c0, int64_t S, int32_t intra) {
    if (intra) return false;
    const int64_t n = 2 * S;
    const int64_t r1 = r0 + kRT < n ? r0 + kRT : n, c1 = c0 + kCT < n ? c0 + kCT : n;
    return (r1 <= S && c1 <= S) || (r0 >= S && c0 >= S);
}

// (m, s): max and sum of exp(. - m) of a set of logits; the empty set is (-inf, 0)
__device__ inline void merge(float &m, float &s, float m2, float s2) {
    const float mm = fmaxf(m, m2);
    if (mm == -INFINITY) return;
    s = s * expf(m - mm) + s2 * expf(m2 - mm);
    m = mm;
}

// ---- forward -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void forward_kernel(int64_t S, int32_t D, float inv_tau, int32_t intra, void *ws,
                                                           float *__restrict__ row_loss_out) {
    __shared__ Stage st;
    __shared__ int32_t col_live[kCT];
    __shared__ float red[2][4][kRT];        // [column half][m, sum, pos, best negative][row]
    const Ws w = ws_of(ws, S, D);
    const int64_t n = 2 * S, r0 = (int64_t)blockIdx.x * kRT;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wr = wv >> 1, wc = wv & 1;
    float m[16], sum[16], pos[16], neg[16];
#pragma unroll
    for (int i = 0; i < 16; i++) {
        m[i] = -INFINITY;
        sum[i] = 0.0f;
        pos[i] = 0.0f;
        neg[i] = -INFINITY;
    }
    for (int64_t c0 = 0; c0 < n; c0 += kCT) {
        if (tile_skipped(r0, c0, S, intra)) continue;
        __syncthreads();
        if (t < kCT) col_live[t] = c0 + t < n ? w.live[c0 + t] : 0;
        f32x16 acc[2];
        logits_tile(w.Z, n, D, r0, c0, st, acc);
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int64_t row = r0 + 32 * wr + 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3);
            const bool row_a = row < S;
            const int64_t partner = row_a ? row + S : row - S;
            float v[2];
            bool in[2];
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int cl = 64 * wc + 32 * j + (lane & 31);
                const int64_t col = c0 + cl;
                v[j] = acc[j][i] * inv_tau;
                in[j] = col_live[cl] != 0 && col != row && (intra || (col < S) != row_a);
                if (col == partner) pos[i] = v[j];
                else if (in[j]) neg[i] = fmaxf(neg[i], v[j]);
            }
            const float mt = fmaxf(in[0] ? v[0] : -INFINITY, in[1] ? v[1] : -INFINITY);
            if (mt > m[i]) {
                sum[i] *= expf(m[i] - mt);
                m[i] = mt;
            }
            if (in[0]) sum[i] += expf(v[0] - m[i]);
            if (in[1]) sum[i] += expf(v[1] - m[i]);
        }
    }
    // the 32 lanes that share a row: a butterfly inside each half of the wave, the same bits in all of them
#pragma unroll
    for (int i = 0; i < 16; i++) {
        for (int x = 1; x <= 16; x <<= 1) {
            const float m2 = __shfl_xor(m[i], x, 64), s2 = __shfl_xor(sum[i], x, 64);
            merge(m[i], sum[i], m2, s2);
            neg[i] = fmaxf(neg[i], __shfl_xor(neg[i], x, 64));
            // (exactly one lane of the row's 64 columns per tile holds the partner; the others hold 0: a sum moves it)
            pos[i] += __shfl_xor(pos[i], x, 64);
        }
        if ((lane & 31) == 0) {
            const int rl = 32 * wr + 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3);
            red[wc][0][rl] = m[i];
            red[wc][1][rl] = sum[i];
            red[wc][2][rl] = pos[i];
            red[wc][3][rl] = neg[i];
        }
    }
    __syncthreads();
    if (t < kRT && r0 + t < n) {
        const int64_t row = r0 + t;
        float mm = red[0][0][t], ss = red[0][1][t];
        merge(mm, ss, red[1][0][t], red[1][1][t]);
        const float p = red[0][2][t] + red[1][2][t];
        const float ng = fmaxf(red[0][3][t], red[1][3][t]);
        const bool live = w.live[row] != 0;
        const double lse = (double)mm + log((double)ss);
        const double rl = live ? lse - (double)p : 0.0;
        w.lse[row] = live ? (float)lse : 0.0f;
        w.row_loss[row] = rl;
        if (row_loss_out) row_loss_out[row] = (float)rl;
        if (live && p >= ng) atomicAdd(&w.head->hits, 1ULL);
    }
}

__global__ __launch_bounds__(kThreads) void loss_partial_kernel(int64_t S, int32_t D, void *ws) {
    __shared__ double v[kThreads];
    const Ws w = ws_of(ws, S, D);
    const int64_t n = 2 * S, r = (int64_t)blockIdx.x * kPart + threadIdx.x;
    v[threadIdx.x] = r < n ? w.row_loss[r] : 0.0;
    for (int h = kThreads / 2; h >= 1; h >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < h) v[threadIdx.x] += v[threadIdx.x + h];
    }
    if (threadIdx.x == 0) w.part[blockIdx.x] = v[0];
}

__global__ void loss_final_kernel(int64_t S, int32_t D, const void *ws, double *loss, int64_t *hits, int64_t *counts) {
    const Ws w = ws_of(const_cast<void *>(ws), S, D);
    const int64_t P = parts_of(2 * S);
    double total = 0.0;
    for (int64_t p = 0; p < P; p++) total += w.part[p];
    const unsigned long long M = w.head->M;
    if (loss) loss[0] = M ? total / (2.0 * (double)M) : 0.0;
    if (hits) hits[0] = (int64_t)w.head->hits;
    if (counts) {
        counts[0] = (int64_t)M;
        counts[1] = (int64_t)w.head->bad;
    }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void backward_kernel(int64_t S, int32_t D, float inv_tau, int32_t intra, void *ws) {
    __shared__ Stage st;
    __shared__ int32_t col_live[kCT];
    __shared__ float col_lse[kCT];
    __shared__ float lw[kRT][kCT + 1];
    const Ws w = ws_of(ws, S, D);
    const int64_t n = 2 * S, r0 = (int64_t)blockIdx.x * kRT;
    const int32_t d0 = (int32_t)blockIdx.y * kDC;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wr = wv >> 1, wc = wv & 1;
    float lse_r[16];
    bool live_r[16];
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int64_t row = r0 + 32 * wr + 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3);
        live_r[i] = row < n && w.live[row] != 0;
        lse_r[i] = live_r[i] ? w.lse[row] : 0.0f;
    }
    f32x16 g[2][2];         // [row half][32 columns of this wave's 64 of G]
#pragma unroll
    for (int i = 0; i < 16; i++) g[0][0][i] = g[0][1][i] = g[1][0][i] = g[1][1][i] = 0.0f;
    const int32_t dcol = d0 + 64 * wv + (lane & 31);
    for (int64_t c0 = 0; c0 < n; c0 += kCT) {
        if (tile_skipped(r0, c0, S, intra)) continue;
        __syncthreads();
        if (t < kCT) {
            const bool in = c0 + t < n;
            col_live[t] = in ? w.live[c0 + t] : 0;
            col_lse[t] = in ? w.lse[c0 + t] : 0.0f;
        }
        f32x16 acc[2];
        logits_tile(w.Z, n, D, r0, c0, st, acc);
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int rl = 32 * wr + 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3);
            const int64_t row = r0 + rl;
            const bool row_a = row < S;
            const int64_t partner = row_a ? row + S : row - S;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int cl = 64 * wc + 32 * j + (lane & 31);
                const int64_t col = c0 + cl;
                const float s = acc[j][i] * inv_tau;
                const bool in = live_r[i] && col_live[cl] != 0 && col != row && (intra || (col < S) != row_a);
                float wt = 0.0f;
                if (in) {
                    wt = expf(s - lse_r[i]) + expf(s - col_lse[cl]);
                    if (col == partner) wt -= 2.0f;
                }
                lw[rl][cl] = wt;
            }
        }
        __syncthreads();
        if (d0 + 64 * wv < D) {        // (uniform per wave)
#pragma unroll 4
            for (int k = 0; k < kCT; k += 2) {
                const int kk = k + (lane >> 5);
                const int64_t col = c0 + kk;
                const float a0 = lw[lane & 31][kk], a1 = lw[32 + (lane & 31)][kk];
                const float *zc = w.Z + (col < n ? col : 0) * D;
                const float b0 = (col < n && dcol < D) ? zc[dcol] : 0.0f;
                const float b1 = (col < n && dcol + 32 < D) ? zc[dcol + 32] : 0.0f;
                g[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, g[0][0], 0, 0, 0);
                g[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, g[0][1], 0, 0, 0);
                g[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, g[1][0], 0, 0, 0);
                g[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, g[1][1], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int rb = 0; rb < 2; rb++)
#pragma unroll
        for (int db = 0; db < 2; db++)
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int64_t row = r0 + 32 * rb + 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3);
                const int32_t d = dcol + 32 * db;
                if (row < n && d < D) w.G[row * D + d] = g[rb][db][i];
            }
}

__global__ __launch_bounds__(kThreads) void finish_kernel(int64_t S, int32_t D, double tau, const void *ws,
                                                          const float *__restrict__ grad_loss, float *__restrict__ dA,
                                                          float *__restrict__ dB) {
    const Ws w = ws_of(const_cast<void *>(ws), S, D);
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (r >= 2 * S) return;
    float *out = r < S ? dA + r * D : dB + (r - S) * D;
    const unsigned long long M = w.head->M;
    if (!w.live[r] || M == 0) {
        for (int32_t d = lane; d < D; d += 64) out[d] = 0.0f;
        return;
    }
    const double coef = (double)grad_loss[0] / (2.0 * (double)M * tau) / w.norm[r];
    const float *z = w.Z + r * D, *gr = w.G + r * D;
    double dot = 0.0;
    for (int32_t d = lane; d < D; d += 64) dot += (double)z[d] * (double)gr[d];
    dot = wave_sum(dot);
    for (int32_t d = lane; d < D; d += 64) out[d] = (float)(coef * ((double)gr[d] - (double)z[d] * dot));
}

int check_shape(const char *who, int64_t S, int32_t D) {
    if (S < 0 || 2 * S >= 2147483648LL) PN_FAIL(PN_ERR_ARG, "%s: %lld pairs, 0 <= 2 S < 2^31", who, (long long)S);
    if (D < 1 || D > kMaxD) PN_FAIL(PN_ERR_ARG, "%s: %d columns, 1 .. %d", who, D, kMaxD);
    return PN_OK;
}

int check_common(const char *who, const float *A, int64_t lda, const float *B, int64_t ldb, int64_t S, int32_t D, double tau,
                 const void *workspace, int64_t workspace_bytes) {
    if (int rc = check_shape(who, S, D)) return rc;
    if (!(tau > 0.0 && tau <= kDblMax)) PN_FAIL(PN_ERR_ARG, "%s: tau %g, finite and > 0", who, tau);
    if (S > 0 && (!A || !B || !workspace)) PN_FAIL(PN_ERR_ARG, "%s: null A, B or workspace", who);
    if (S > 0 && (lda < D || ldb < D)) PN_FAIL(PN_ERR_ARG, "%s: row strides %lld / %lld below D = %d", who, (long long)lda,
                                               (long long)ldb, D);
    if (workspace_bytes < ws_bytes(S, D))
        PN_FAIL(PN_ERR_ARG, "%s: workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes,
                (long long)ws_bytes(S, D));
    if (S > 0 && ((uintptr_t)workspace & 7)) PN_FAIL(PN_ERR_ARG, "%s: workspace not 8-byte aligned", who);
    return PN_OK;
}

}  // namespace

extern "C" {

int pn_contrast_workspace_bytes(int64_t S, int32_t D, int64_t *bytes) {
    if (!bytes) PN_FAIL(PN_ERR_ARG, "pn_contrast_workspace_bytes: null result");
    if (int rc = check_shape("pn_contrast_workspace_bytes", S, D)) return rc;
    *bytes = ws_bytes(S, D);
    return PN_OK;
}

int pn_contrast_tiles(int32_t out[3]) {
    if (!out) PN_FAIL(PN_ERR_ARG, "pn_contrast_tiles: null result");
    out[0] = kRT;
    out[1] = kCT;
    out[2] = kKC;
    return PN_OK;
}

int pn_contrast_forward(pn_context *ctx, const float *A, int64_t lda, const float *B, int64_t ldb, int64_t S, int32_t D,
                        double tau, int32_t intra, const uint8_t *valid, void *workspace, int64_t workspace_bytes,
                        const pn_contrast_out *out, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_common("pn_contrast_forward", A, lda, B, ldb, S, D, tau, workspace, workspace_bytes)) return rc;
    if (!out) PN_FAIL(PN_ERR_ARG, "pn_contrast_forward: null output description");
    if (int rc = pn::context_check_device(ctx)) return rc;
    if (S == 0) {       // no kernel: loss, hits and counts zero
        if (out->loss) PN_CHECK_HIP(hipMemsetAsync(out->loss, 0, sizeof(double), stream));
        if (out->hits) PN_CHECK_HIP(hipMemsetAsync(out->hits, 0, sizeof(int64_t), stream));
        if (out->counts) PN_CHECK_HIP(hipMemsetAsync(out->counts, 0, 2 * sizeof(int64_t), stream));
        return PN_OK;
    }
    const int64_t n = 2 * S;
    const dim3 block(kThreads);
    PN_CHECK_HIP(hipMemsetAsync(workspace, 0, sizeof(Header), stream));
    hipLaunchKernelGGL(prep_kernel, dim3((unsigned)((S + 3) / 4)), block, 0, stream, A, lda, B, ldb, S, D, valid, workspace);
    hipLaunchKernelGGL(forward_kernel, dim3((unsigned)((n + kRT - 1) / kRT)), block, 0, stream, S, D, (float)(1.0 / tau),
                       intra ? 1 : 0, workspace, out->row_loss);
    hipLaunchKernelGGL(loss_partial_kernel, dim3((unsigned)parts_of(n)), block, 0, stream, S, D, workspace);
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(1), 0, stream, S, D, (const void *)workspace, out->loss, out->hits,
                       out->counts);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int pn_contrast_backward(pn_context *ctx, const float *A, int64_t lda, const float *B, int64_t ldb, int64_t S, int32_t D,
                         double tau, int32_t intra, void *workspace, int64_t workspace_bytes, const float *grad_loss, float *dA,
                         float *dB, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_common("pn_contrast_backward", A, lda, B, ldb, S, D, tau, workspace, workspace_bytes)) return rc;
    if (S > 0 && (!grad_loss || !dA || !dB)) PN_FAIL(PN_ERR_ARG, "pn_contrast_backward: null grad_loss, dA or dB");
    if (int rc = pn::context_check_device(ctx)) return rc;
    if (S == 0) return PN_OK;
    const int64_t n = 2 * S;
    const dim3 block(kThreads);
    hipLaunchKernelGGL(backward_kernel, dim3((unsigned)((n + kRT - 1) / kRT), (unsigned)((D + kDC - 1) / kDC)), block, 0, stream,
                       S, D, (float)(1.0 / tau), intra ? 1 : 0, workspace);
    hipLaunchKernelGGL(finish_kernel, dim3((unsigned)((n + 3) / 4)), block, 0, stream, S, D, tau, (const void *)workspace,
                       grad_loss, dA, dB);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

}  // extern "C"
