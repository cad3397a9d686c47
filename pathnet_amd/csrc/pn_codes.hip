// pn_codes.hip -- distance codes and walk checks for caller-supplied paths (pn_path_codes).
//
// The walker emits a node's distance code while it walks (pn_sampler.hip).  Paths that come from elsewhere -- another
// sampler, an ids-only file, paths sampled before edges were hidden or added, rows whose target node is not their first
// node -- carry ids only.  These kernels annotate them from the walker's own hop source and count what is wrong with them:
//     codes[s, w, t] = min(hops(source(s) -> ids[s, w, t]), L - 1)
// over the directed edges the tables were built from, with three counters (ids outside the graph, steps that are no
// edge, nodes further than L - 1 hops from their row's source) and the flat index of the first id outside the graph.
// An id outside the graph never indexes a table.
//
//   path_codes_dense_kernel: one lane per path element, one byte gathered from dis[source][x] and one from
//     dis[x][next] (1 = the node itself, 2 = an edge).
//   path_codes_otf_kernel: one wavefront per row.  The out-ball of the row's source goes into the wave's LDS hash table
//     ONCE (pn_otf.h, the walker's table: radius 2, or 1 / 0 when a hub's ball would overflow it) and serves the row's
//     W * L queries, one per lane.  The walker knows that the node at step t is at most t hops away and searches below
//     that bound; here nothing is known, so a query deepens level by level up to L - 1 - rf:
//       x == source -> 0;  x in the ball -> its level;  else for k = 1, 2, ..: is there a chain x <- c1 <- ... <- ck of
//       in-neighbours whose last node is in the ball?  The first k that has one gives hops = k + rf, exactly: a shortest
//       path of length d > rf has its rf-th node on the ball's outermost level and the later ones outside the ball, so it
//       is found at k = d - rf; every chain found is a real path, so nothing shorter is reported; and with the complete
//       ball of radius rf no chain can end on an inner level before a shorter one ended on the outermost.  This holds for
//       rf = 2, 1 and 0 alike, so the hub fallbacks stay exact; no chain up to k = L - 1 - rf means "far".
//     Two prunings, neither of which can drop a shortest path: (a) chains that repeat a node within two steps (self loops,
//     a <- b <- a) are not followed -- shortest paths are simple; (b) the in-list of the chain's last-but-one node is
//     scanned only when the Bloom filter over the out-neighbours of the ball's outermost level says "maybe" (no false
//     negatives).  The search keeps no visited set: its cost grows with the number of in-neighbour chains of length
//     L - 1 - rf, which is small for sparse graphs and L <= 8 but is not bounded by the graph's size.
//   Both kernels sum their counters per wave, then per workgroup in LDS, and issue one atomic per workgroup and counter;
//   first_bad is an unsigned 64-bit atomicMin on a word initialised to all ones, which read as int64 is the "none" of -1.
#include <hip/hip_runtime.h>

#include "pn_internal.h"
#include "pn_otf.h"

namespace {

constexpr int kCodesThreads = 256;
constexpr int64_t kReportScratchBytes = 256;     // the counters of a call without a report go to the workspace
constexpr unsigned long long kNone = ~0ull;

struct CodesParams {
    int32_t n;
    const uint8_t *dis;
    const int64_t *adj_off;
    const int32_t *adj;
    const int64_t *radj_off;
    const int32_t *radj;
    int32_t W, L, rows;
    const int32_t *ids;
    const int32_t *sources;
    uint8_t *codes;
    unsigned long long *report;      // {out_of_range, non_edges, far, first_bad}
};

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o);
        v = w < v ? w : v;
    }
    return v;
}

// the counts of this thread -> wave -> workgroup (LDS) -> one atomic per counter.  Every thread of the workgroup calls it.
__device__ __forceinline__ void report_counts(const CodesParams &p, unsigned oor, unsigned non_edge, unsigned far,
                                              unsigned long long first, unsigned *s_sum, unsigned long long *s_first) {
    oor = wave_sum(oor);
    non_edge = wave_sum(non_edge);
    far = wave_sum(far);
    first = wave_min(first);
    if ((threadIdx.x & 63) == 0) {
        if (oor) atomicAdd(&s_sum[0], oor);
        if (non_edge) atomicAdd(&s_sum[1], non_edge);
        if (far) atomicAdd(&s_sum[2], far);
        if (first != kNone) atomicMin(s_first, first);
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_sum[threadIdx.x]) atomicAdd(&p.report[threadIdx.x], (unsigned long long)s_sum[threadIdx.x]);
    if (threadIdx.x == 3 && *s_first != kNone) atomicMin(&p.report[3], *s_first);
}

__global__ __launch_bounds__(kCodesThreads) void path_codes_dense_kernel(CodesParams p) {
    __shared__ unsigned s_sum[3];
    __shared__ unsigned long long s_first;
    if (threadIdx.x < 3) s_sum[threadIdx.x] = 0;
    if (threadIdx.x == 3) s_first = kNone;
    __syncthreads();
    const int64_t per_row = (int64_t)p.W * p.L;
    const int64_t total = per_row * p.rows;
    const int64_t e = (int64_t)blockIdx.x * kCodesThreads + threadIdx.x;
    unsigned oor = 0, non_edge = 0, far = 0;
    if (e < total) {
        const int64_t row = e / per_row;
        const int32_t x = p.ids[e];
        const int32_t src = p.sources ? p.sources[row] : p.ids[row * per_row];
        const bool x_ok = (uint32_t)x < (uint32_t)p.n;
        int code = p.L - 1;
        if (!x_ok) {
            oor = 1;
        } else if ((uint32_t)src >= (uint32_t)p.n) {
            far = 1;                                            // no source in the graph: nothing is reachable
        } else {
            const int b = p.dis[(size_t)src * (size_t)p.n + (size_t)x];      // 0 = unreached, else hops + 1
            if (b == 0 || b > p.L)
                far = 1;
            else
                code = b - 1;
        }
        p.codes[e] = (uint8_t)code;
        if (x_ok && (int32_t)(e % p.L) + 1 < p.L) {
            const int32_t y = p.ids[e + 1];
            if ((uint32_t)y < (uint32_t)p.n) {
                const int b = p.dis[(size_t)x * (size_t)p.n + (size_t)y];
                non_edge = !(b == 1 || b == 2);
            }
        }
    }
    report_counts(p, oor, non_edge, far, oor ? (unsigned long long)e : kNone, s_sum, &s_first);
}

// is y in the sorted out-list of x?
__device__ __forceinline__ bool otf_has_edge(const CodesParams &p, int32_t x, int32_t y) {
    int64_t lo = p.adj_off[x], hi = p.adj_off[x + 1];
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int32_t a = p.adj[mid];
        if (a == y) return true;
        if (a < y)
            lo = mid + 1;
        else
            hi = mid;
    }
    return false;
}

__global__ __launch_bounds__(kOtfWaves * 64) void path_codes_otf_kernel(CodesParams p) {
    // the walker's LDS budget: table 8 KB + stack 4 KB + Bloom filter 4 KB per wave
    __shared__ uint32_t s_tab[kOtfWaves][kOtfCap];
    __shared__ int s_cnt[kOtfWaves];
    __shared__ uint32_t s_stack[kOtfWaves][2][kOtfMaxDepth][64];   // per lane cursor / end per level (positions in radj);
                                                                    // before the queries: the list of the ball's outermost level
    __shared__ uint32_t s_bloom[kOtfWaves][kOtfBloomWords];
    __shared__ unsigned s_sum[3];
    __shared__ unsigned long long s_first;
    if (threadIdx.x < 3) s_sum[threadIdx.x] = 0;
    if (threadIdx.x == 3) s_first = kNone;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#define CUR(d_) s_stack[wave][0][d_][lane]
#define END(d_) s_stack[wave][1][d_][lane]
    uint32_t *tab = s_tab[wave];
    uint32_t *bloom = s_bloom[wave];
    const int64_t per_row = (int64_t)p.W * p.L;
    unsigned oor = 0, non_edge = 0, far = 0;
    unsigned long long first = kNone;
    // rows of this wave (wave-uniform loop; no workgroup barrier inside)
    for (int64_t row = (int64_t)blockIdx.x * kOtfWaves + wave; row < p.rows; row += (int64_t)gridDim.x * kOtfWaves) {
        const int32_t src = p.sources ? p.sources[row] : p.ids[row * per_row];
        const bool src_ok = (uint32_t)src < (uint32_t)p.n;
        int rf = 0;
        if (src_ok) {
            rf = otf_build_ball(tab, &s_cnt[wave], lane, src, p.adj_off, p.adj);
            if (p.L - 1 - rf >= 1)      // a search can happen
                otf_build_bloom(bloom, tab, &s_cnt[wave], &s_stack[wave][0][0][0], lane, (uint32_t)rf, p.adj_off, p.adj);
        }
        const int kmax = p.L - 1 - rf;
        for (int64_t q = lane; q < per_row; q += 64) {
            const int64_t e = row * per_row + q;
            const int32_t x = p.ids[e];
            const bool x_ok = (uint32_t)x < (uint32_t)p.n;
            int hops = -1;                                      // -1: further than L - 1, or unreachable
            if (!x_ok) {
                oor++;
                if (first == kNone) first = (unsigned long long)e;      // (q ascends: the lane's first)
            } else if (src_ok) {
                if (x == src) {
                    hops = 0;
                } else if ((hops = otf_lookup(tab, x)) >= 0) {
                    if (hops > p.L - 1) hops = -1;              // the ball is built to radius 2 whatever L is: L <= 2
                } else {
                    for (int k = 1; k <= kmax && hops < 0; k++) {
                        // chains x = c0 <- c1 <- ... <- ck with ck in the ball; level lvl scans the in-list of c_lvl
                        if (k == 1 && !otf_bloom_maybe(bloom, x)) continue;
                        int lvl = 0;
                        int32_t nd = x, gp = -1;                // the node whose in-list is scanned, and the one before it
                        CUR(0) = (uint32_t)p.radj_off[x];
                        END(0) = (uint32_t)p.radj_off[x + 1];
                        while (lvl >= 0) {
                            const uint32_t cur = CUR(lvl);
                            if (cur >= END(lvl)) {
                                lvl--;
                                if (lvl >= 0) {
                                    nd = lvl == 0 ? x : p.radj[CUR(lvl - 1) - 1];
                                    gp = lvl == 0 ? -1 : lvl == 1 ? x : p.radj[CUR(lvl - 2) - 1];
                                }
                                continue;
                            }
                            CUR(lvl) = cur + 1;
                            const int32_t c = p.radj[cur];
                            if (lvl + 1 == k) {
                                const int dc = otf_lookup(tab, c);
                                if (dc >= 0) {
                                    hops = k + dc;
                                    break;
                                }
                            } else if (c != nd && c != gp && c != x && (lvl + 2 < k || otf_bloom_maybe(bloom, c))) {
                                gp = nd;
                                nd = c;
                                lvl++;
                                CUR(lvl) = (uint32_t)p.radj_off[c];
                                END(lvl) = (uint32_t)p.radj_off[c + 1];
                            }
                        }
                    }
                }
            }
            if (x_ok && hops < 0) far++;
            p.codes[e] = (uint8_t)(hops < 0 ? p.L - 1 : hops);
            if (x_ok && (int32_t)(q % p.L) + 1 < p.L) {
                const int32_t y = p.ids[e + 1];
                if ((uint32_t)y < (uint32_t)p.n && y != x && !otf_has_edge(p, x, y)) non_edge++;
            }
        }
        __builtin_amdgcn_wave_barrier();        // the next row rebuilds the table, the list and the filter
    }
#undef CUR
#undef END
    report_counts(p, oor, non_edge, far, first, s_sum, &s_first);
}

int check_args(const pn_sampler_tables *tb, int32_t W, int32_t L, int32_t rows, bool *otf) {
    if (!tb) PN_FAIL(PN_ERR_ARG, "pn_path_codes: null tables");
    if (tb->n < 1 || W < 1 || L < 1 || rows < 0)
        PN_FAIL(PN_ERR_ARG, "pn_path_codes: bad shape (n=%d W=%d L=%d rows=%d)", tb->n, W, L, rows);
    if (L > 254) PN_FAIL(PN_ERR_ARG, "pn_path_codes: L = %d (a code is one byte and the dense table holds hops + 1)", L);
    *otf = tb->dis == nullptr;
    if (*otf && (!tb->adj_off || !tb->adj || !tb->radj_off || !tb->radj))
        PN_FAIL(PN_ERR_ARG, "pn_path_codes: neither a dense hop table nor the CSR lists for on-the-fly hop codes");
    if (*otf && (tb->n >= (1 << 28) || L > 8))
        PN_FAIL(PN_ERR_ARG, "on-the-fly hop codes support n < 2^28 and L <= 8 (n=%d L=%d)", tb->n, L);
    return PN_OK;
}

}  // namespace

extern "C" {

int pn_path_codes_workspace_bytes(const pn_sampler_tables *tb, int32_t W, int32_t L, int32_t rows, int64_t *bytes) {
    bool otf;
    if (!bytes) PN_FAIL(PN_ERR_ARG, "pn_path_codes_workspace_bytes: null result");
    if (int rc = check_args(tb, W, L, rows, &otf)) return rc;
    *bytes = kReportScratchBytes;
    return PN_OK;
}

int pn_path_codes(pn_context *ctx, const pn_sampler_tables *tb, int32_t W, int32_t L, int32_t rows, const int32_t *ids,
                  const int32_t *sources, uint8_t *codes, pn_path_report *report, void *workspace, int64_t workspace_bytes,
                  void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    bool otf;
    if (int rc = check_args(tb, W, L, rows, &otf)) return rc;
    if (rows > 0 && (!ids || !codes)) PN_FAIL(PN_ERR_ARG, "pn_path_codes: null ids or codes");
    if (!workspace || workspace_bytes < kReportScratchBytes)
        PN_FAIL(PN_ERR_ARG, "pn_path_codes: workspace holds %lld bytes, need %lld", (long long)workspace_bytes,
                (long long)kReportScratchBytes);
    const int64_t total = (int64_t)rows * W * L;
    if (total / kCodesThreads + 1 > 2147483647LL) PN_FAIL(PN_ERR_ARG, "pn_path_codes: too many path elements for one launch");
    if (int rc = pn::context_check_device(ctx)) return rc;

    CodesParams cp{};
    cp.n = tb->n;
    cp.dis = tb->dis;
    cp.adj_off = tb->adj_off;
    cp.adj = tb->adj;
    cp.radj_off = tb->radj_off;
    cp.radj = tb->radj;
    cp.W = W;
    cp.L = L;
    cp.rows = rows;
    cp.ids = ids;
    cp.sources = sources;
    cp.codes = codes;
    cp.report = reinterpret_cast<unsigned long long *>(report ? (void *)report : workspace);
    // counters = 0, first_bad = -1 (all ones: the identity of the unsigned atomicMin)
    PN_CHECK_HIP(hipMemsetAsync(cp.report, 0, 3 * sizeof(unsigned long long), stream));
    PN_CHECK_HIP(hipMemsetAsync(cp.report + 3, 0xFF, sizeof(unsigned long long), stream));
    if (total == 0) return PN_OK;
    if (otf) {
        const int64_t blocks = ((int64_t)rows + kOtfWaves - 1) / kOtfWaves;
        hipLaunchKernelGGL(path_codes_otf_kernel, dim3((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20))),
                           dim3(kOtfWaves * 64), 0, stream, cp);
    } else {
        hipLaunchKernelGGL(path_codes_dense_kernel, dim3((unsigned)((total + kCodesThreads - 1) / kCodesThreads)),
                           dim3(kCodesThreads), 0, stream, cp);
    }
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

}  // extern "C"
