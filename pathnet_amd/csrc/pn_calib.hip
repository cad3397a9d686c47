// pn_calib.hip -- calibration of ensemble predictions: the temperature sweep (pn_calib_sweep) and the calibration statistics
// of a finished prediction (pn_calib_stats).  The scaled ensemble add, pn_ensemble_add_scaled, lives beside the plain one in
// pn_ensemble.hip.
//
//   sweep_rows_kernel<G>    logits [R, S, C] fp32, target, temps [T] -> row_nll [S, T] fp64.  The work unit is the (row, t)
//                           pair: ONE group of G threads owns it (G by C, pn_group.h), takes the R samples in ascending r
//                           and sums the classes in pn_group.h's order, so a row's values do not depend on where the row sits.
//   sweep_partial_kernel    rows [256 p, 256 p + 256) of every column, added in ascending s -> part [P, T]
//   sweep_final_kernel      part in ascending p -> nll [T]; counts, best, tau
//   stats_rows_kernel       a thread per row, 256 rows per workgroup: reliability bins (integer atomics, gathered in LDS
//                           first), the row's -log p[target] and Brier term (classes in ascending c), the sort key
//   stats_blocksum / stats_finish / stats_scan / stats_aurc
//                           errors along the sorted order -> err_prefix, aurc; the fp64 partials in ascending order
//
// Every fp64 sum over rows is a sum of fixed-size partials (256 rows, a halving tree over the 256 slots, slots past the
// end holding 0) combined in ascending order by one thread: an order that depends on the row count alone.  No floating-point
// atomic.  Plain C++ and vector stores only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pn_group.h"
#include "pn_internal.h"

namespace {

using namespace pn::group;

constexpr int kPart = 256;               // rows per partial of a column sum (= kThreads)
constexpr int kMaxT = 256;
constexpr int kMaxBins = 1024;
constexpr double kDblMax = 1.7976931348623157e308;
constexpr int32_t kUnusedKey = 2147483647;

static_assert(kPart == kThreads, "a partial is what one workgroup holds");

__host__ __device__ inline int64_t parts_of(int64_t n) { return (n + kPart - 1) / kPart; }
__host__ __device__ inline int64_t round8(int64_t b) { return (b + 7) & ~(int64_t)7; }
__device__ inline bool finite_positive(double t) { return t > 0.0 && t <= kDblMax; }

// the sum of the 256 slots of `v` as a halving tree (128, 64, ..., 1); every thread of the workgroup makes the call
__device__ inline double tree_sum(double *v) {
    for (int h = kThreads / 2; h >= 1; h >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < h) v[threadIdx.x] += v[threadIdx.x + h];
    }
    __syncthreads();
    const double out = v[0];
    __syncthreads();
    return out;
}

// ---- sweep ---------------------------------------------------------------------------------------------------------------------
struct SweepWs {
    double *row_nll;        // [S, T]
    double *part;           // [P, T]
    int32_t *flag;          // [S]     0 used, 1 target outside [0, C), 2 no finite sample
    int32_t *pcnt;          // [P, 3]  rows of each flag in a partial
};

__host__ __device__ inline SweepWs sweep_ws(void *base, int64_t S, int32_t T) {
    SweepWs w;
    const int64_t P = parts_of(S);
    char *p = (char *)base;
    w.row_nll = (double *)p;
    p += sizeof(double) * (size_t)S * T;
    w.part = (double *)p;
    p += sizeof(double) * (size_t)P * T;
    w.flag = (int32_t *)p;
    p += sizeof(int32_t) * (size_t)S;
    w.pcnt = (int32_t *)p;
    return w;
}

inline int64_t sweep_ws_bytes(int64_t S, int32_t T) {
    const int64_t P = parts_of(S);
    return round8(8 * S * T + 8 * P * T + 4 * S + 12 * P);
}

template <int G>
__global__ __launch_bounds__(kThreads) void sweep_rows_kernel(const float *__restrict__ logits, int32_t R, int64_t S, int32_t C,
                                                               const int64_t *__restrict__ target,
                                                               const double *__restrict__ temps, int32_t T, void *ws) {
    __shared__ RedSlots red;
    const SweepWs w = sweep_ws(ws, S, T);
    const int lane = G == 1 ? 0 : (int)(threadIdx.x % G);
    const int64_t per_block = kThreads / G;
    const int64_t pairs = S * T;
    // (the pair, and with it every `continue`, is the same for all G threads of a group: the barriers of G = 256 stay paired)
    for (int64_t pair = (int64_t)blockIdx.x * per_block + threadIdx.x / G; pair < pairs;
         pair += (int64_t)gridDim.x * per_block) {
        const int64_t s = pair / T;
        const int32_t t = (int32_t)(pair - s * T);
        const int64_t y = target[s];
        if (y < 0 || y >= C) {
            if (lane == 0) {
                w.row_nll[pair] = 0.0;
                if (t == 0) w.flag[s] = 1;
            }
            continue;
        }
        const double temp = temps[t];
        const bool t_ok = finite_positive(temp);
        const double inv = t_ok ? 1.0 / temp : 1.0;        // (a refused temperature still counts the row's finite samples)
        double acc = 0.0;
        int32_t n_ok = 0;
        for (int32_t r = 0; r < R; r++) {
            const float *x = logits + ((int64_t)r * S + s) * C;
            Best<float> b{-INFINITY, C, 0};
            for (int32_t c = lane; c < C; c += G) {
                const float v = x[c];
                if (finite_f32(v)) best_merge(b, v, c, 0);
                else b.flag = 1;
            }
            b = group_best<G>(b, red.bf);
            if (b.flag) continue;
            const double m = (double)b.key;
            double z = 0.0;
            for (int32_t c = lane; c < C; c += G) z += exp(((double)x[c] - m) * inv);
            z = group_sum<G>(z, red.d);
            acc += exp(((double)x[y] - m) * inv) / z;
            n_ok += 1;
        }
        if (lane == 0) {
            w.row_nll[pair] = (t_ok && n_ok > 0) ? -log(acc / (double)n_ok) : 0.0;
            if (t == 0) w.flag[s] = n_ok > 0 ? 0 : 2;
        }
    }
}

// workgroup p, thread t: part[p, t] = sum of row_nll[s, t] over the partial's rows in ascending s
__global__ __launch_bounds__(kThreads) void sweep_partial_kernel(int64_t S, int32_t T, void *ws) {
    __shared__ int32_t cnt[3];
    const SweepWs w = sweep_ws(ws, S, T);
    const int64_t P = parts_of(S);
    for (int64_t p = blockIdx.x; p < P; p += gridDim.x) {
        const int64_t s0 = p * kPart;
        const int64_t s1 = s0 + kPart < S ? s0 + kPart : S;
        if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
        __syncthreads();
        if (s0 + threadIdx.x < s1) atomicAdd(&cnt[w.flag[s0 + threadIdx.x]], 1);
        if ((int32_t)threadIdx.x < T) {
            double v = 0.0;
            for (int64_t s = s0; s < s1; s++) v += w.row_nll[s * T + threadIdx.x];
            w.part[p * T + threadIdx.x] = v;
        }
        __syncthreads();
        if (threadIdx.x < 3) w.pcnt[p * 3 + threadIdx.x] = cnt[threadIdx.x];
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void sweep_final_kernel(int64_t S, int32_t T, const double *__restrict__ temps,
                                                                const void *ws, double *nll, int32_t *best, double *tau,
                                                                int64_t *counts) {
    __shared__ double col[kMaxT];
    __shared__ int64_t used;
    const SweepWs w = sweep_ws(const_cast<void *>(ws), S, T);
    const int64_t P = parts_of(S);
    const int32_t t = (int32_t)threadIdx.x;
    if (t < T) {
        double v = 0.0;
        for (int64_t p = 0; p < P; p++) v += w.part[p * T + t];
        if (!finite_positive(temps[t])) v = INFINITY;
        col[t] = v;
        if (nll) nll[t] = v;
    }
    if (t < 3) {
        int64_t n = 0;
        for (int64_t p = 0; p < P; p++) n += w.pcnt[p * 3 + t];
        if (counts) counts[t] = n;
        if (t == 0) used = n;
    }
    __syncthreads();
    if (t == 0) {
        int32_t at = -1;
        if (used > 0)
            for (int32_t i = 0; i < T; i++)
                if (fabs(col[i]) <= kDblMax && (at < 0 || col[i] < col[at])) at = i;
        if (best) best[0] = at;
        if (tau) tau[0] = at >= 0 ? temps[at] : 1.0;
    }
}

// ---- statistics ----------------------------------------------------------------------------------------------------------------
struct StatsWs {
    double *part_nll;       // [P]
    double *part_brier;     // [P]
    double *part_aurc;      // [P]
    int64_t *used;          // [1]  rows used in this call (m)
    int32_t *part_used;     // [P]
    int32_t *blk;           // [P]  errors of a partial of the sorted order, then their exclusive scan
    int32_t *keys_in;       // [n]
    int32_t *keys_out;      // [n]
    int32_t *vals_in;       // [n]
    int32_t *err;           // [n]  1: a used row whose label is not its target
    void *sort_tmp;
};

__host__ __device__ inline StatsWs stats_ws(void *base, int64_t n) {
    StatsWs w;
    const int64_t P = parts_of(n);
    char *p = (char *)base;
    w.part_nll = (double *)p;
    p += sizeof(double) * (size_t)P;
    w.part_brier = (double *)p;
    p += sizeof(double) * (size_t)P;
    w.part_aurc = (double *)p;
    p += sizeof(double) * (size_t)P;
    w.used = (int64_t *)p;
    p += sizeof(int64_t);
    w.part_used = (int32_t *)p;
    p += sizeof(int32_t) * (size_t)P;
    w.blk = (int32_t *)p;
    p += sizeof(int32_t) * (size_t)P;
    w.keys_in = (int32_t *)p;
    p += sizeof(int32_t) * (size_t)n;
    w.keys_out = (int32_t *)p;
    p += sizeof(int32_t) * (size_t)n;
    w.vals_in = (int32_t *)p;
    p += sizeof(int32_t) * (size_t)n;
    w.err = (int32_t *)p;
    p += sizeof(int32_t) * (size_t)n;
    w.sort_tmp = (void *)(((uintptr_t)p + 255) & ~(uintptr_t)255);
    return w;
}

inline int64_t stats_fixed_bytes(int64_t n) { return 24 * parts_of(n) + 8 + 8 * parts_of(n) + 16 * n + 256; }

struct StatsParams {
    int64_t n;
    int32_t C, B;
    const float *conf;
    const int64_t *label;
    const int64_t *target;
    const float *prob;
    pn_calib_stats_out o;
    void *ws;
};

enum { CNT_USED = 0, CNT_NO_LABEL, CNT_BAD_TARGET, CNT_BAD_CONF, CNT_ZERO_PROB, CNT_N };

__global__ __launch_bounds__(kThreads) void stats_rows_kernel(StatsParams sp) {
    __shared__ unsigned long long bins[3][kMaxBins];
    __shared__ double red_nll[kThreads], red_brier[kThreads];
    __shared__ int32_t cnt[CNT_N];
    const StatsWs w = stats_ws(sp.ws, sp.n);
    const int64_t P = parts_of(sp.n);
    const int32_t B = sp.B, C = sp.C;
    for (int64_t p = blockIdx.x; p < P; p += gridDim.x) {
        for (int32_t b = threadIdx.x; b < B; b += kThreads) bins[0][b] = bins[1][b] = bins[2][b] = 0ULL;
        if (threadIdx.x < CNT_N) cnt[threadIdx.x] = 0;
        __syncthreads();
        const int64_t i = p * kPart + threadIdx.x;
        double t_nll = 0.0, t_brier = 0.0;
        if (i < sp.n) {
            const float cf = sp.conf[i];
            const int64_t lab = sp.label[i], y = sp.target[i];
            const int reason = lab < 0 ? CNT_NO_LABEL
                                       : (y < 0 || y >= C) ? CNT_BAD_TARGET : !(cf >= 0.0f && cf <= 1.0f) ? CNT_BAD_CONF : CNT_USED;
            atomicAdd(&cnt[reason], 1);
            int32_t key = kUnusedKey, wrong = 0;
            if (reason == CNT_USED) {
                const double cd = (double)cf;
                int32_t b = (int32_t)floor(cd * (double)B);
                b = b < B - 1 ? b : B - 1;
                wrong = lab != y;
                atomicAdd(&bins[0][b], 1ULL);
                atomicAdd(&bins[1][b], (unsigned long long)(1 - wrong));
                atomicAdd(&bins[2][b], (unsigned long long)llrint(cd * 4294967296.0));
                key = 0x3F800000 - (cf == 0.0f ? 0 : __float_as_int(cf));      // (-0.0 sorts as 0.0)
                if (sp.prob) {
                    const float *q = sp.prob + i * C;
                    const float py = q[y];
                    if (py > 0.0f) t_nll = -log((double)py);
                    else atomicAdd(&cnt[CNT_ZERO_PROB], 1);
                    for (int32_t c = 0; c < C; c++) {
                        const double d = (double)q[c] - (c == y ? 1.0 : 0.0);
                        t_brier += d * d;
                    }
                }
            }
            w.keys_in[i] = key;
            w.vals_in[i] = (int32_t)i;
            w.err[i] = wrong;
        }
        red_nll[threadIdx.x] = t_nll;
        red_brier[threadIdx.x] = t_brier;
        const double s_nll = tree_sum(red_nll), s_brier = tree_sum(red_brier);      // (barriers: the LDS adds above are done)
        if (threadIdx.x == 0) {
            w.part_nll[p] = s_nll;
            w.part_brier[p] = s_brier;
            w.part_used[p] = cnt[CNT_USED];
        }
        for (int32_t b = threadIdx.x; b < B; b += kThreads) {
            if (bins[0][b] == 0ULL) continue;
            atomicAdd((unsigned long long *)&sp.o.bin_count[b], bins[0][b]);
            if (bins[1][b]) atomicAdd((unsigned long long *)&sp.o.bin_correct[b], bins[1][b]);
            if (bins[2][b]) atomicAdd((unsigned long long *)&sp.o.bin_conf[b], bins[2][b]);
        }
        if (threadIdx.x < CNT_N && sp.o.counts && cnt[threadIdx.x])
            atomicAdd((unsigned long long *)&sp.o.counts[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
        __syncthreads();
    }
}

// blk[p] = errors among positions [256 p, 256 p + 256) of the sorted order
__global__ __launch_bounds__(kThreads) void stats_blocksum_kernel(int64_t n, const int32_t *__restrict__ order, void *ws) {
    __shared__ int32_t total;
    const StatsWs w = stats_ws(ws, n);
    const int64_t P = parts_of(n);
    for (int64_t p = blockIdx.x; p < P; p += gridDim.x) {
        if (threadIdx.x == 0) total = 0;
        __syncthreads();
        const int64_t k = p * kPart + threadIdx.x;
        if (k < n && w.err[order[k]]) atomicAdd(&total, 1);
        __syncthreads();
        if (threadIdx.x == 0) w.blk[p] = total;
        __syncthreads();
    }
}

// one workgroup: the fp64 partials in ascending order into sums, m, and blk -> its exclusive scan
__global__ __launch_bounds__(kThreads) void stats_finish_kernel(int64_t n, int with_prob, int with_curve, double *sums, void *ws) {
    __shared__ int32_t scan[kThreads];
    __shared__ int32_t carry;
    const StatsWs w = stats_ws(ws, n);
    const int64_t P = parts_of(n);
    if (with_prob && sums && threadIdx.x < 2) {
        const double *part = threadIdx.x == 0 ? w.part_nll : w.part_brier;
        double v = 0.0;
        for (int64_t p = 0; p < P; p++) v += part[p];
        sums[threadIdx.x] += v;
    }
    if (threadIdx.x == 64) {       // (another wave than the two fp64 sums)
        int64_t m = 0;
        for (int64_t p = 0; p < P; p++) m += w.part_used[p];
        w.used[0] = m;
    }
    if (!with_curve) return;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t p0 = 0; p0 < P; p0 += kThreads) {      // (integers: any order gives the same scan)
        const int64_t p = p0 + threadIdx.x;
        const int32_t mine = p < P ? w.blk[p] : 0;
        scan[threadIdx.x] = mine;
        __syncthreads();
        for (int d = 1; d < kThreads; d <<= 1) {
            const int32_t add = (int)threadIdx.x >= d ? scan[threadIdx.x - d] : 0;
            __syncthreads();
            scan[threadIdx.x] += add;
            __syncthreads();
        }
        if (p < P) w.blk[p] = carry + scan[threadIdx.x] - mine;
        __syncthreads();
        if (threadIdx.x == 0) carry += scan[kThreads - 1];
        __syncthreads();
    }
}

// err_prefix[k] = errors among the first k + 1 rows of the order; part_aurc[p] = sum of err_prefix[k] / (k + 1) over k < m
__global__ __launch_bounds__(kThreads) void stats_scan_kernel(int64_t n, const int32_t *__restrict__ order, int32_t *err_prefix,
                                                               void *ws) {
    __shared__ int32_t scan[kThreads];
    __shared__ double red[kThreads];
    const StatsWs w = stats_ws(ws, n);
    const int64_t P = parts_of(n);
    const int64_t m = w.used[0];
    for (int64_t p = blockIdx.x; p < P; p += gridDim.x) {
        const int64_t k = p * kPart + threadIdx.x;
        scan[threadIdx.x] = k < n ? w.err[order[k]] : 0;
        __syncthreads();
        for (int d = 1; d < kThreads; d <<= 1) {
            const int32_t add = (int)threadIdx.x >= d ? scan[threadIdx.x - d] : 0;
            __syncthreads();
            scan[threadIdx.x] += add;
            __syncthreads();
        }
        const int32_t e = w.blk[p] + scan[threadIdx.x];
        if (k < n && err_prefix) err_prefix[k] = e;
        red[threadIdx.x] = k < m ? (double)e / (double)(k + 1) : 0.0;
        const double v = tree_sum(red);
        if (threadIdx.x == 0) w.part_aurc[p] = v;
    }
}

__global__ void stats_aurc_kernel(int64_t n, double *aurc, const void *ws) {
    const StatsWs w = stats_ws(const_cast<void *>(ws), n);
    const int64_t P = parts_of(n);
    const int64_t m = w.used[0];
    double v = 0.0;
    for (int64_t p = 0; p < P; p++) v += w.part_aurc[p];
    aurc[0] = m > 0 ? v / (double)m : 0.0;
}

unsigned part_blocks(int64_t n) {
    const int64_t P = parts_of(n);
    return (unsigned)(P < kMaxBlocks ? P : kMaxBlocks);
}

int check_sweep_shape(const char *who, int64_t S, int32_t T) {
    if (S < 0 || S > 2147483647LL) PN_FAIL(PN_ERR_ARG, "%s: %lld rows, 0 .. 2^31 - 1", who, (long long)S);
    if (T < 1 || T > kMaxT) PN_FAIL(PN_ERR_ARG, "%s: %d temperatures, 1 .. %d", who, T, kMaxT);
    return PN_OK;
}

int check_stats_shape(const char *who, int64_t n, int32_t B) {
    if (n < 0 || n > 2000000000LL) PN_FAIL(PN_ERR_ARG, "%s: %lld rows, 0 .. 2 000 000 000", who, (long long)n);
    if (B < 1 || B > kMaxBins) PN_FAIL(PN_ERR_ARG, "%s: %d bins, 1 .. %d", who, B, kMaxBins);
    return PN_OK;
}

}  // namespace

extern "C" {

int pn_calib_sweep_workspace_bytes(int64_t S, int32_t T, int64_t *bytes) {
    if (!bytes) PN_FAIL(PN_ERR_ARG, "pn_calib_sweep_workspace_bytes: null result");
    if (int rc = check_sweep_shape("pn_calib_sweep_workspace_bytes", S, T)) return rc;
    *bytes = sweep_ws_bytes(S, T);
    return PN_OK;
}

int pn_calib_sweep(pn_context *ctx, const float *logits, int32_t R, int64_t S, int32_t C, const int64_t *target,
                   const double *temps, int32_t T, void *workspace, int64_t workspace_bytes, const pn_calib_sweep_out *out,
                   void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_sweep_shape("pn_calib_sweep", S, T)) return rc;
    if (C < 1 || C > kMaxC) PN_FAIL(PN_ERR_ARG, "pn_calib_sweep: %d classes, 1 .. %d", C, kMaxC);
    if (R < 1) PN_FAIL(PN_ERR_ARG, "pn_calib_sweep: %d samples, at least 1", R);
    if (!out) PN_FAIL(PN_ERR_ARG, "pn_calib_sweep: null output description");
    if (!temps) PN_FAIL(PN_ERR_ARG, "pn_calib_sweep: null temps");
    if (S > 0 && (!logits || !target || !workspace)) PN_FAIL(PN_ERR_ARG, "pn_calib_sweep: null logits, target or workspace");
    if (workspace_bytes < sweep_ws_bytes(S, T))
        PN_FAIL(PN_ERR_ARG, "pn_calib_sweep: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)sweep_ws_bytes(S, T));
    if (S > 0 && ((uintptr_t)workspace & 7)) PN_FAIL(PN_ERR_ARG, "pn_calib_sweep: workspace not 8-byte aligned");
    if (int rc = pn::context_check_device(ctx)) return rc;
    if (S == 0) {       // no kernel: best = -1, tau = 1.0, nll and counts zero
        if (out->nll) PN_CHECK_HIP(hipMemsetAsync(out->nll, 0, sizeof(double) * (size_t)T, stream));
        if (out->counts) PN_CHECK_HIP(hipMemsetAsync(out->counts, 0, sizeof(int64_t) * 3, stream));
        if (out->best) PN_CHECK_HIP(hipMemsetAsync(out->best, 0xFF, sizeof(int32_t), stream));
        if (out->tau) {
            PN_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)out->tau, 0, 1, stream));
            PN_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)((char *)out->tau + 4), 0x3FF00000, 1, stream));
        }
        return PN_OK;
    }
    const int G = group_of(C);
    const dim3 grid(blocks_for(S * T, G)), block(kThreads);
    if (G == 1)
        hipLaunchKernelGGL(sweep_rows_kernel<1>, grid, block, 0, stream, logits, R, S, C, target, temps, T, workspace);
    else if (G == 64)
        hipLaunchKernelGGL(sweep_rows_kernel<64>, grid, block, 0, stream, logits, R, S, C, target, temps, T, workspace);
    else
        hipLaunchKernelGGL(sweep_rows_kernel<256>, grid, block, 0, stream, logits, R, S, C, target, temps, T, workspace);
    hipLaunchKernelGGL(sweep_partial_kernel, dim3(part_blocks(S)), block, 0, stream, S, T, workspace);
    hipLaunchKernelGGL(sweep_final_kernel, dim3(1), block, 0, stream, S, T, temps, (const void *)workspace, out->nll, out->best,
                       out->tau, out->counts);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int pn_calib_stats_workspace_bytes(int64_t n, int32_t B, int64_t *bytes) {
    if (!bytes) PN_FAIL(PN_ERR_ARG, "pn_calib_stats_workspace_bytes: null result");
    if (int rc = check_stats_shape("pn_calib_stats_workspace_bytes", n, B)) return rc;
    *bytes = round8(stats_fixed_bytes(n) + (int64_t)pn::sort_temp_reserve(n));
    return PN_OK;
}

int pn_calib_stats(pn_context *ctx, const float *confidence, const int64_t *label, const int64_t *target, const float *prob,
                   int64_t n, int32_t C, int32_t B, void *workspace, int64_t workspace_bytes, const pn_calib_stats_out *out,
                   void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_stats_shape("pn_calib_stats", n, B)) return rc;
    if (C < 1 || C > kMaxC) PN_FAIL(PN_ERR_ARG, "pn_calib_stats: %d classes, 1 .. %d", C, kMaxC);
    if (!out) PN_FAIL(PN_ERR_ARG, "pn_calib_stats: null output description");
    if (!out->bin_count || !out->bin_correct || !out->bin_conf) PN_FAIL(PN_ERR_ARG, "pn_calib_stats: null bin arrays");
    if (prob && !out->sums) PN_FAIL(PN_ERR_ARG, "pn_calib_stats: prob without sums");
    const bool curve = out->order != nullptr;
    if (!curve && (out->err_prefix || out->aurc)) PN_FAIL(PN_ERR_ARG, "pn_calib_stats: err_prefix / aurc asked for without order");
    if (n > 0 && (!confidence || !label || !target || !workspace))
        PN_FAIL(PN_ERR_ARG, "pn_calib_stats: null confidence, label, target or workspace");
    const int64_t need = round8(stats_fixed_bytes(n) + (int64_t)pn::sort_temp_reserve(n));
    if (workspace_bytes < need)
        PN_FAIL(PN_ERR_ARG, "pn_calib_stats: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
    if (n > 0 && ((uintptr_t)workspace & 7)) PN_FAIL(PN_ERR_ARG, "pn_calib_stats: workspace not 8-byte aligned");
    if (int rc = pn::context_check_device(ctx)) return rc;
    if (n == 0) {
        if (out->aurc) PN_CHECK_HIP(hipMemsetAsync(out->aurc, 0, sizeof(double), stream));
        return PN_OK;
    }
    StatsParams sp{};
    sp.n = n;
    sp.C = C;
    sp.B = B;
    sp.conf = confidence;
    sp.label = label;
    sp.target = target;
    sp.prob = prob;
    sp.o = *out;
    sp.ws = workspace;
    const dim3 grid(part_blocks(n)), block(kThreads);
    hipLaunchKernelGGL(stats_rows_kernel, grid, block, 0, stream, sp);
    PN_CHECK_HIP(hipGetLastError());
    if (curve) {
        const StatsWs w = stats_ws(workspace, n);
        const size_t tmp_bytes = (size_t)((char *)workspace + workspace_bytes - (char *)w.sort_tmp);
        if (int rc = pn::sort_pairs_i32(w.sort_tmp, tmp_bytes, w.keys_in, w.keys_out, w.vals_in, out->order, n, 31, stream_))
            return rc;
        hipLaunchKernelGGL(stats_blocksum_kernel, grid, block, 0, stream, n, (const int32_t *)out->order, workspace);
    }
    hipLaunchKernelGGL(stats_finish_kernel, dim3(1), block, 0, stream, n, prob ? 1 : 0, curve ? 1 : 0, out->sums, workspace);
    if (curve) {
        hipLaunchKernelGGL(stats_scan_kernel, grid, block, 0, stream, n, (const int32_t *)out->order, out->err_prefix, workspace);
        if (out->aurc) hipLaunchKernelGGL(stats_aurc_kernel, dim3(1), dim3(1), 0, stream, n, out->aurc, (const void *)workspace);
    }
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

}  // extern "C"
