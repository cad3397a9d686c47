// pn_explain_units.hip -- the units of a node or edge explanation (pn_explain_units / pn_explain_node_totals).
//
// pn_explain_overlap (pn_explain.hip) removes the members that carry a label; this file makes the labels.  A row's W members
// consumed L nodes each: the row's distinct nodes (or undirected edges of consecutive steps) are its units, and every step is
// told which of them it touched (include/pathnet_hip.h has the definition).
//
//   units_kernel          one workgroup owns a row.  The row's n = W * M <= 1024 keys (int64; "no unit" is the largest int64,
//                         above every key) go into LDS twice: in step order, and padded to a power of two for a bitonic sort
//                         (at most 55 compare-exchange rounds of 512 pairs).  A sorted key that differs from its left
//                         neighbour opens a unit; the units' positions are a prefix count over the sorted array (four keys a
//                         thread, then a scan over the 256 threads); every step finds its key among the row's units by
//                         bisection.  No workspace, integers only: the result is a function of the row alone.
//   node_totals_kernel    one workgroup owns a listed row: every qualifying unit adds into the per-node table with 64-bit
//                         integer atomics (exact, any order), and the row's best unit -- largest drop_delta, lowest position
//                         among equals -- is found by a wave butterfly and one pass over the four waves' results.
// Plain C++ and vector stores only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pn_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1 << 16;      // rows beyond that are taken in a grid-stride loop
constexpr int kMaxKeys = 1024;           // W * M
constexpr int kMaxL = 16;
constexpr int kMaxG = 1024;
constexpr long long kNoKey = 0x7fffffffffffffffLL;       // above (2^31 - 1) << 32 | (2^31 - 1), the largest edge key

__device__ inline bool finite32(float v) { return fabsf(v) <= 3.4028234663852886e38f; }

__global__ __launch_bounds__(kThreads) void units_kernel(int64_t S, int32_t W, int32_t L, int32_t kind, const int32_t *node,
                                                         const int32_t *exclude, int64_t *unit, int32_t *count, int32_t *label) {
    __shared__ long long key[kMaxKeys];          // in step order
    __shared__ long long srt[kMaxKeys];          // sorted; then the units, packed to the front
    __shared__ int32_t scan[2][kThreads];
    const int tid = threadIdx.x;
    const int32_t M = kind == PN_UNIT_EDGE ? L - 1 : L, n = W * M;
    int32_t np2 = 1;
    while (np2 < n) np2 <<= 1;
    for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
        const int32_t *row = node + s * W * L;
        const int32_t ex = exclude ? exclude[s] : -1;          // (a negative id is no unit anyway)
        for (int32_t i = tid; i < np2; i += kThreads) {
            long long k = kNoKey;
            if (i < n) {
                const int32_t j = i / M, m = i - j * M;
                if (kind == PN_UNIT_EDGE) {
                    const int32_t a = row[j * L + m], b = row[j * L + m + 1];
                    if (a >= 0 && b >= 0) k = ((long long)(a < b ? a : b) << 32) | (long long)(a < b ? b : a);
                } else {
                    const int32_t a = row[j * L + m];
                    if (a >= 0 && a != ex) k = a;
                }
                key[i] = k;
            }
            srt[i] = k;
        }
        __syncthreads();
        // ---- bitonic sort of srt[0 .. np2), ascending -------------------------------------------------------------------
        for (int32_t size = 2; size <= np2; size <<= 1) {
            for (int32_t stride = size >> 1; stride >= 1; stride >>= 1) {
                for (int32_t t = tid; t < (np2 >> 1); t += kThreads) {
                    const int32_t lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                    const bool up = (lo & size) == 0;
                    const long long a = srt[lo], b = srt[hi];
                    if ((a > b) == up) {
                        srt[lo] = b;
                        srt[hi] = a;
                    }
                }
                __syncthreads();
            }
        }
        // ---- the units: a sorted key that differs from its left neighbour; thread t owns srt[4 t .. 4 t + 4) ------------------
        long long mine[4];
        int32_t head[4], heads = 0;
#pragma unroll
        for (int32_t k = 0; k < 4; k++) {
            const int32_t i = 4 * tid + k;
            mine[k] = i < np2 ? srt[i] : kNoKey;
            head[k] = i < np2 && mine[k] != kNoKey && (i == 0 || srt[i - 1] != mine[k]);
            heads += head[k];
        }
        scan[0][tid] = heads;
        __syncthreads();                                      // (also: every thread holds its keys before srt is rewritten)
        int32_t cur = 0;
        for (int32_t d = 1; d < kThreads; d <<= 1) {
            scan[cur ^ 1][tid] = scan[cur][tid] + (tid >= d ? scan[cur][tid - d] : 0);
            cur ^= 1;
            __syncthreads();
        }
        const int32_t total = scan[cur][kThreads - 1];
        int32_t pos = scan[cur][tid] - heads;
#pragma unroll
        for (int32_t k = 0; k < 4; k++)
            if (head[k]) srt[pos++] = mine[k];
        __syncthreads();
        // ---- outputs ---------------------------------------------------------------------------------------------------------
        for (int32_t i = tid; i < n; i += kThreads) {
            unit[s * n + i] = i < total ? srt[i] : -1;
            const long long k = key[i];
            int32_t lb = -1;
            if (k != kNoKey) {
                int32_t lo = 0, hi = total - 1;              // the key is among the units
                while (lo < hi) {
                    const int32_t mid = (lo + hi) >> 1;
                    if (srt[mid] < k) lo = mid + 1;
                    else hi = mid;
                }
                lb = lo;
            }
            label[s * n + i] = lb;
        }
        if (tid == 0) count[s] = total;
        __syncthreads();        // the next row reuses the LDS
    }
}

__global__ __launch_bounds__(kThreads) void node_totals_kernel(int64_t S, int32_t G, int32_t N, const int64_t *unit,
                                                               const float *drop_delta, const float *keep_gain,
                                                               const uint8_t *flip, const int32_t *present, const int32_t *rows,
                                                               int64_t n, unsigned long long *table) {
    __shared__ float sv[kThreads / 64];
    __shared__ int32_t sg[kThreads / 64];
    unsigned long long *rows_present = table, *members = table + N, *flips = members + N, *top = flips + N;
    const int tid = threadIdx.x;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const int64_t row = rows ? (int64_t)rows[i] : i;
        if (row < 0 || row >= S) continue;                  // (the whole workgroup takes the same turn)
        float best = 0.0f;
        int32_t best_g = G;                                  // G: nothing yet
        for (int32_t g = tid; g < G; g += kThreads) {
            const int64_t u = unit[row * G + g];
            const int32_t pr = present[row * G + g];
            const float fd = drop_delta[row * G + g], fk = keep_gain[row * G + g];
            if (u < 0 || u >= N || pr <= 0 || !finite32(fd) || !finite32(fk)) continue;
            atomicAdd(rows_present + u, 1ULL);
            atomicAdd(members + u, (unsigned long long)pr);
            if (flip[row * G + g]) atomicAdd(flips + u, 1ULL);
            if (best_g == G || fd > best) {                  // (ascending g within a thread: the first of equals stays)
                best = fd;
                best_g = g;
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float v2 = __shfl_xor(best, m, 64);
            const int32_t g2 = __shfl_xor(best_g, m, 64);
            if (g2 != G && (best_g == G || v2 > best || (v2 == best && g2 < best_g))) {
                best = v2;
                best_g = g2;
            }
        }
        if ((tid & 63) == 0) {
            sv[tid >> 6] = best;
            sg[tid >> 6] = best_g;
        }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < kThreads / 64; w++) {
                const float v2 = sv[w];
                const int32_t g2 = sg[w];
                if (g2 != G && (best_g == G || v2 > best || (v2 == best && g2 < best_g))) {
                    best = v2;
                    best_g = g2;
                }
            }
            if (best_g != G) atomicAdd(top + unit[row * G + best_g], 1ULL);
        }
        __syncthreads();        // sv / sg are rewritten for the next row
    }
}

unsigned blocks_for(int64_t n) { return (unsigned)(n < kMaxBlocks ? n : kMaxBlocks); }

}  // namespace

extern "C" {

int pn_explain_units(pn_context *ctx, int64_t S, int32_t W, int32_t L, int32_t kind, const int32_t *node, const int32_t *exclude,
                     int64_t *unit, int32_t *count, int32_t *label, void *stream) {
    if (kind != PN_UNIT_NODE && kind != PN_UNIT_EDGE) PN_FAIL(PN_ERR_ARG, "pn_explain_units: kind %d", kind);
    if (S < 0 || S > 2147483647LL) PN_FAIL(PN_ERR_ARG, "pn_explain_units: %lld rows, 0 .. 2^31 - 1", (long long)S);
    if (W < 1) PN_FAIL(PN_ERR_ARG, "pn_explain_units: %d members, at least 1", W);
    if (L < (kind == PN_UNIT_EDGE ? 2 : 1) || L > kMaxL)
        PN_FAIL(PN_ERR_ARG, "pn_explain_units: %d steps, %d .. %d", L, kind == PN_UNIT_EDGE ? 2 : 1, kMaxL);
    const int64_t M = kind == PN_UNIT_EDGE ? L - 1 : L;
    if (W * M > kMaxKeys)
        PN_FAIL(PN_ERR_ARG, "pn_explain_units: W * M = %lld keys per row, at most %d", (long long)(W * M), kMaxKeys);
    if (kind == PN_UNIT_EDGE && exclude) PN_FAIL(PN_ERR_ARG, "pn_explain_units: exclude is for PN_UNIT_NODE only");
    if (S > 0 && (!node || !unit || !count || !label)) PN_FAIL(PN_ERR_ARG, "pn_explain_units: null node, unit, count or label");
    if (int rc = pn::context_check_device(ctx)) return rc;
    if (S == 0) return PN_OK;
    hipLaunchKernelGGL(units_kernel, dim3(blocks_for(S)), dim3(kThreads), 0, (hipStream_t)stream, S, W, L, kind, node, exclude,
                       unit, count, label);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int pn_explain_node_totals(pn_context *ctx, int64_t S, int32_t G, int32_t N, const int64_t *unit, const float *drop_delta,
                           const float *keep_gain, const uint8_t *flip, const int32_t *present, const int32_t *rows,
                           int64_t n_rows, int64_t *table, void *stream) {
    if (S < 0 || S > 2147483647LL) PN_FAIL(PN_ERR_ARG, "pn_explain_node_totals: %lld rows, 0 .. 2^31 - 1", (long long)S);
    if (G < 1 || G > kMaxG) PN_FAIL(PN_ERR_ARG, "pn_explain_node_totals: %d units per row, 1 .. %d", G, kMaxG);
    if (N < 1) PN_FAIL(PN_ERR_ARG, "pn_explain_node_totals: %d nodes, at least 1", N);
    if (n_rows < 0 || n_rows > 2147483647LL || (!rows && n_rows != 0))
        PN_FAIL(PN_ERR_ARG, "pn_explain_node_totals: %lld listed rows%s", (long long)n_rows, rows ? "" : " without a list");
    const int64_t n = rows ? n_rows : S;
    if (n > 0 && S > 0 && (!unit || !drop_delta || !keep_gain || !flip || !present || !table))
        PN_FAIL(PN_ERR_ARG, "pn_explain_node_totals: null unit, drop_delta, keep_gain, flip, present or table");
    if (int rc = pn::context_check_device(ctx)) return rc;
    if (n == 0 || S == 0) return PN_OK;
    hipLaunchKernelGGL(node_totals_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, (hipStream_t)stream, S, G, N, unit, drop_delta,
                       keep_gain, flip, present, rows, n, (unsigned long long *)table);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

}  // extern "C"
