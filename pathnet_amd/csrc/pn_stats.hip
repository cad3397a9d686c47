// pn_stats.hip -- walk statistics (pn_walk_stats): what sampled paths look like, counted where they are.
//
// One pass over ids int32 [rows, W, L] and codes uint8 [rows, W, L]; a row is the W paths of one (epoch, source node).
// Everything is an integer count, so the result depends neither on the launch geometry nor on the order of the atomics.
//
//   walk_stats_kernel: G threads own a row -- one wavefront (G = 64) while W * L <= kWaveRowMax, so that a workgroup holds
//     four rows (a Cornell row is 160 entries), else the whole workgroup (G = 256).  The workgroup strides over the rows;
//     per row:
//       stage     the row's ids go into LDS once; every later phase reads them there
//       elements  one entry per thread and turn: code-by-step, label pair of (source, node), stay / back against the
//                 one or two entries before it, visits; the counts go into the workgroup's int32 LDS tables
//       paths     one path per thread and turn: its distinct ids by comparing every entry with the ones before it
//                 (L <= 16: at most 120 LDS reads)
//       unique    the W path indices are sorted in LDS by lexicographic comparison of the id sequences (bitonic network,
//                 exact: no hashing), and the boundaries between unequal neighbours counted
//       cover     the staged ids are then sorted in place the same way and the boundaries counted
//     The sorting network is the ascending-only form (first step of a merge pairs i with i ^ (k - 1), the others with
//     i ^ j); with it the missing entries of a length that is no power of two act as +infinity at the top and are simply
//     skipped, so ids need no sentinel value: -1, n and 2^31 - 1 are ordinary integers here.
//     The threads of a row meet between the phases and between the steps of a sort (row_sync): a workgroup barrier when
//     the workgroup owns the row -- every loop around one has a trip count that depends on W and L alone, and a workgroup
//     without a row left never enters the loop --, and nothing but a compiler fence when a wavefront owns it, so the four
//     rows of a workgroup do not wait for each other.
//     At the end the workgroup adds the non-zero entries of its LDS tables to the caller's int64 tables, one 64-bit
//     atomicAdd each.  label_pairs is held in LDS while L * C * C <= kLabelPairsLds; a larger table takes one global
//     atomic per entry of the paths instead.  visits [n] is always global: one atomic per entry at a step >= 1.
//   stats_zero_kernel: clears the global tables of a call that does not accumulate, in one launch.
//   path_mult_kernel (pn_path_multiplicity): how often each path of a row occurs in it, as weights for the aggregators' pooling.
// LDS per workgroup: (W * L + W / 2 + 2) words per row slot and L * L + 4 L + 3 (+ L * C * C) words of tables:
// 3.3 KB at Cornell's shape, 59 KB at the largest.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pn_internal.h"

namespace {

constexpr int kStatsThreads = 256;
constexpr int kWaveRowMax = 1024;         // entries of a row one wavefront takes: 16 per lane
constexpr int kLabelPairsLds = 2048;      // L * C * C up to here is counted in LDS
constexpr int kMaxEntries = 8192;         // W * L: 32 KB of staged ids
constexpr int kMaxBlocks = 2048;          // 256 CUs x 8 resident workgroups
constexpr int kZeroTables = 8;

typedef unsigned long long u64;

struct StatsParams {
    int32_t n, W, L, C;
    int64_t rows;
    const int32_t *ids;
    const uint8_t *codes;
    const int32_t *sources;
    const int32_t *labels;
    pn_walk_stats_out o;
    int32_t G;              // threads per row: 64 or 256
    int32_t lp_lds;         // words of label_pairs held in LDS (0: counted with global atomics, or not wanted)
};

struct ZeroTabs {
    int64_t *ptr[kZeroTables];
    int64_t count[kZeroTables];
    int k;
};

__global__ __launch_bounds__(kStatsThreads) void stats_zero_kernel(ZeroTabs z) {
    for (int t = 0; t < z.k; t++)
        for (int64_t i = blockIdx.x * (int64_t)kStatsThreads + threadIdx.x; i < z.count[t];
             i += (int64_t)gridDim.x * kStatsThreads)
            z.ptr[t][i] = 0;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// -1 / 0 / 1: the id sequences of paths x and y of the staged row, lexicographically from the LAST step backwards -- any total
// order puts equal sequences side by side, and the paths of a row share their first node, so this one decides sooner
__device__ __forceinline__ int path_cmp(const int32_t *a, int L, int x, int y) {
    const int32_t *px = a + x * L, *py = a + y * L;
    for (int t = L - 1; t >= 0; t--) {
        const int32_t u = px[t], v = py[t];
        if (u != v) return u < v ? -1 : 1;
    }
    return 0;
}

// the pair (i, i2) with i < i2 that pair number q exchanges in a step of the ascending-only bitonic network: the first step
// of the merge into runs of k (j == 0) mirrors the lower half of a run onto the upper, the others (j = k/4 .. 1) pair i with
// i + j
__device__ __forceinline__ void network_pair(int q, int k, int j, int *i, int *i2) {
    if (j == 0) {
        const int half = k >> 1, r = q & (half - 1), base = (q - r) << 1;
        *i = base + r;
        *i2 = base + k - 1 - r;
    } else {
        const int r = q & (j - 1);
        *i = ((q - r) << 1) + r;
        *i2 = *i + j;
    }
}

// the G threads of a row meet.  A wavefront's LDS accesses are served in program order, so a row that one wavefront owns
// needs the compiler kept from moving them and no hardware barrier: the four rows of a workgroup then run independently.
__device__ __forceinline__ void row_sync(int G) {
    if (G == 64) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}

// sorts n entries (n2: the power of two that holds n) with the network; `exchange(i, i2)` orders the pair so that the smaller
// entry is at i.  Called by every thread of the workgroup: the barriers do not depend on `act`.
template <class Exchange>
__device__ __forceinline__ void network_sort(int n, int n2, int lt, int G, bool act, Exchange exchange) {
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = 0;; j = j ? j >> 1 : k >> 2) {
            row_sync(G);
            if (act)
                for (int q = lt; q < (n2 >> 1); q += G) {
                    int i, i2;
                    network_pair(q, k, j, &i, &i2);
                    if (i2 < n) exchange(i, i2);
                }
            if (j == 1 || k == 2) break;      // (a merge into runs of 2 is the mirror step alone)
        }
    row_sync(G);
}

__device__ __forceinline__ void add64(int64_t *dst, int32_t v) {
    if (v) atomicAdd(reinterpret_cast<u64 *>(dst), (u64)(uint32_t)v);
}

__global__ __launch_bounds__(kStatsThreads) void walk_stats_kernel(StatsParams p) {
    extern __shared__ int32_t smem[];
    const int L = p.L, W = p.W, WL = W * L, G = p.G;
    const int sub = threadIdx.x / G, lt = threadIdx.x - sub * G, rpb = kStatsThreads / G;
    // the workgroup's tables
    int32_t *h_sc = smem;                 // [L][L]
    int32_t *h_stay = h_sc + L * L;       // [L]
    int32_t *h_back = h_stay + L;         // [L]
    int32_t *h_unl = h_back + L;          // [L]
    int32_t *h_dh = h_unl + L;            // [L + 1]
    int32_t *h_cnt = h_dh + L + 1;        // {out_of_range, bad_codes}
    int32_t *h_lp = h_cnt + 2;            // [L][C][C] when lp_lds
    const int tables = L * L + 4 * L + 3 + p.lp_lds;
    // this row slot
    const int slot_words = WL + (W + 1) / 2 + 2;
    int32_t *a = smem + tables + sub * slot_words;                      // [W][L] staged ids
    uint16_t *idx = reinterpret_cast<uint16_t *>(a + WL);               // [W] path indices
    int32_t *rc = a + WL + (W + 1) / 2;                                 // {unique paths, cover}
    for (int i = threadIdx.x; i < tables; i += kStatsThreads) smem[i] = 0;

    int wl2 = 1, w2 = 1;                  // the powers of two that hold W * L and W
    while (wl2 < WL) wl2 <<= 1;
    while (w2 < W) w2 <<= 1;
    const bool want_lp = p.labels && p.o.label_pairs, want_unl = p.labels && p.o.unlabeled;

    __syncthreads();                      // the tables are cleared
    for (int64_t base = (int64_t)blockIdx.x * rpb; base < p.rows; base += (int64_t)gridDim.x * rpb) {
        const int64_t row = base + sub;
        const bool act = row < p.rows;
        const int64_t at = row * WL;
        row_sync(G);                      // the slot's last row is done with
        if (act)
            for (int e = lt; e < WL; e += G) a[e] = p.ids[at + e];
        if (lt < 2) rc[lt] = 0;
        row_sync(G);
        if (act) {
            // ---- elements
            const int32_t src = p.sources ? p.sources[row] : a[0];
            int la = -1;                  // the source's label, -1: none
            if (p.labels && (uint32_t)src < (uint32_t)p.n) {
                const int32_t l = p.labels[src];
                if ((uint32_t)l < (uint32_t)p.C) la = l;
            }
            for (int e = lt; e < WL; e += G) {
                const int t = e % L;
                const int32_t x = a[e];
                const int d = p.codes[at + e];
                const bool in = (uint32_t)x < (uint32_t)p.n;
                if (!in) atomicAdd(&h_cnt[0], 1);
                if (d >= L) {
                    atomicAdd(&h_cnt[1], 1);
                } else {
                    atomicAdd(&h_sc[t * L + d], 1);
                    if (want_lp || want_unl) {
                        int lb = -1;
                        if (in && la >= 0) {
                            const int32_t l = p.labels[x];
                            if ((uint32_t)l < (uint32_t)p.C) lb = l;
                        }
                        if (lb < 0) {
                            atomicAdd(&h_unl[d], 1);
                        } else if (want_lp) {
                            const int at_lp = (d * p.C + la) * p.C + lb;
                            if (p.lp_lds)
                                atomicAdd(&h_lp[at_lp], 1);
                            else
                                atomicAdd(reinterpret_cast<u64 *>(p.o.label_pairs) + at_lp, 1ull);
                        }
                    }
                }
                if (t >= 1) {
                    const int32_t x1 = a[e - 1];
                    if (x == x1)
                        atomicAdd(&h_stay[t], 1);
                    else if (t >= 2 && x == a[e - 2])
                        atomicAdd(&h_back[t], 1);
                    if (in && p.o.visits) atomicAdd(reinterpret_cast<u64 *>(p.o.visits) + x, 1ull);
                }
            }
            // ---- paths: distinct ids of each
            if (p.o.distinct_hist)
                for (int w = lt; w < W; w += G) {
                    const int32_t *px = a + w * L;
                    int k = 0;
                    for (int t = 0; t < L; t++) {
                        const int32_t x = px[t];
                        bool seen = false;
                        for (int j = 0; j < t; j++) seen |= px[j] == x;
                        k += !seen;
                    }
                    atomicAdd(&h_dh[k], 1);
                }
        }
        // ---- unique: distinct id sequences among the W paths
        if (p.o.unique_paths) {
            if (act)
                for (int w = lt; w < W; w += G) idx[w] = (uint16_t)w;
            network_sort(W, w2, lt, G, act, [&](int i, int i2) {
                const uint16_t x = idx[i], y = idx[i2];
                if (path_cmp(a, L, x, y) > 0) {
                    idx[i] = y;
                    idx[i2] = x;
                }
            });
            int c = 0;
            if (act)
                for (int w = lt; w < W; w += G) c += w == 0 || path_cmp(a, L, idx[w - 1], idx[w]) != 0;
            c = wave_sum_i(c);
            if ((threadIdx.x & 63) == 0 && c) atomicAdd(&rc[0], c);
        }
        // ---- cover: distinct ids among the W * L entries (sorts the staged ids: nothing reads them in path order after this)
        if (p.o.cover) {
            network_sort(WL, wl2, lt, G, act, [&](int i, int i2) {
                const int32_t x = a[i], y = a[i2];
                if (x > y) {
                    a[i] = y;
                    a[i2] = x;
                }
            });
            int c = 0;
            if (act)
                for (int e = lt; e < WL; e += G) c += e == 0 || a[e - 1] != a[e];
            c = wave_sum_i(c);
            if ((threadIdx.x & 63) == 0 && c) atomicAdd(&rc[1], c);
        }
        row_sync(G);
        if (act && lt == 0) {
            if (p.o.unique_paths) p.o.unique_paths[row] = rc[0];
            if (p.o.cover) p.o.cover[row] = rc[1];
        }
    }
    __syncthreads();                      // every row slot has added its last counts
    // ---- the workgroup's tables -> the caller's
    for (int i = threadIdx.x; i < tables; i += kStatsThreads) {
        const int32_t v = smem[i];
        if (!v) continue;
        int r = i;
        if (r < L * L) {
            if (p.o.step_code) add64(p.o.step_code + r, v);
            continue;
        }
        r -= L * L;
        if (r < L) {
            if (p.o.stay) add64(p.o.stay + r, v);
            continue;
        }
        r -= L;
        if (r < L) {
            if (p.o.back) add64(p.o.back + r, v);
            continue;
        }
        r -= L;
        if (r < L) {
            if (p.o.unlabeled) add64(p.o.unlabeled + r, v);
            continue;
        }
        r -= L;
        if (r < L + 1) {
            if (p.o.distinct_hist) add64(p.o.distinct_hist + r, v);
            continue;
        }
        r -= L + 1;
        if (r < 2) {
            if (p.o.counters) add64(p.o.counters + r, v);
            continue;
        }
        r -= 2;
        add64(p.o.label_pairs + r, v);        // (lp_lds > 0 only when the table is wanted)
    }
}

// ---- path multiplicities (pn_path_multiplicity) -----------------------------------------------------------------------------
// mult[r, j] = paths of row r whose id sequence (and code sequence, with codes) equals path j's when j is the first of them,
// else 0.  A workgroup per row, striding over the rows: the row's ids (and codes) are staged in LDS, a thread per path compares
// its path with every path of the row -- W * W * L LDS reads, 6 400 at W = 40, L = 4; the unique-path count's sort would save
// nothing at that size.  Integer counts written as floats (<= W <= 8192: exact).
__global__ __launch_bounds__(kStatsThreads) void path_mult_kernel(int W, int L, int64_t rows, const int32_t *__restrict__ ids,
                                                                  const uint8_t *__restrict__ codes, float *__restrict__ mult) {
    extern __shared__ int32_t smem[];
    const int WL = W * L;
    int32_t *a = smem;                                              // [W][L] ids
    uint8_t *cd = reinterpret_cast<uint8_t *>(smem + WL);           // [W][L] codes (with codes)
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int64_t at = row * WL;
        __syncthreads();                  // the last row is done with
        for (int e = threadIdx.x; e < WL; e += kStatsThreads) {
            a[e] = ids[at + e];
            if (codes) cd[e] = codes[at + e];
        }
        __syncthreads();
        for (int j = threadIdx.x; j < W; j += kStatsThreads) {
            int count = 0;
            bool first = true;
            for (int k = 0; k < W; k++) {
                bool eq = true;
                for (int t = L - 1; t >= 0 && eq; t--) eq = a[j * L + t] == a[k * L + t];
                if (codes)
                    for (int t = 0; t < L && eq; t++) eq = cd[j * L + t] == cd[k * L + t];
                count += eq;
                first = first && !(eq && k < j);
            }
            mult[row * W + j] = first ? (float)count : 0.0f;
        }
    }
}

int check_shape(const char *who, int32_t n, int32_t W, int32_t L, int64_t rows, int32_t C) {
    if (n < 1 || W < 1 || L < 1 || rows < 0)
        PN_FAIL(PN_ERR_ARG, "%s: bad shape (n=%d W=%d L=%d rows=%lld)", who, n, W, L, (long long)rows);
    if (L > 16) PN_FAIL(PN_ERR_ARG, "%s: L = %d, at most 16", who, L);
    if ((int64_t)W * L > kMaxEntries)
        PN_FAIL(PN_ERR_ARG, "%s: W * L = %lld entries in a row, at most %d", who, (long long)W * L, kMaxEntries);
    if (C < 0 || C > 64) PN_FAIL(PN_ERR_ARG, "%s: %d classes, at most 64", who, C);
    return PN_OK;
}

}  // namespace

extern "C" {

int pn_walk_stats_workspace_bytes(int32_t n, int32_t W, int32_t L, int64_t rows, int32_t C, int64_t *bytes) {
    if (!bytes) PN_FAIL(PN_ERR_ARG, "pn_walk_stats_workspace_bytes: null result");
    if (int rc = check_shape("pn_walk_stats_workspace_bytes", n, W, L, rows, C)) return rc;
    *bytes = 0;         // a row is counted in LDS and the tables are the caller's: nothing is kept in between
    return PN_OK;
}

int pn_walk_stats(pn_context *ctx, int32_t n, int32_t W, int32_t L, int64_t rows, const int32_t *ids,
                  const uint8_t *codes, const int32_t *sources, const int32_t *labels, int32_t C, int32_t accumulate,
                  const pn_walk_stats_out *out, void *workspace, int64_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_shape("pn_walk_stats", n, W, L, rows, labels ? C : 0)) return rc;
    if (labels && C < 1) PN_FAIL(PN_ERR_ARG, "pn_walk_stats: labels with %d classes, need 1..64", C);
    if (!out) PN_FAIL(PN_ERR_ARG, "pn_walk_stats: null output description");
    if (!labels && (out->label_pairs || out->unlabeled))
        PN_FAIL(PN_ERR_ARG, "pn_walk_stats: label_pairs / unlabeled asked for without labels");
    if (rows > 0 && (!ids || !codes)) PN_FAIL(PN_ERR_ARG, "pn_walk_stats: null ids or codes");
    if (workspace_bytes < 0) PN_FAIL(PN_ERR_ARG, "pn_walk_stats: workspace of %lld bytes", (long long)workspace_bytes);
    (void)workspace;    // the query says 0
    StatsParams sp{};
    sp.n = n;
    sp.W = W;
    sp.L = L;
    sp.C = labels ? C : 0;
    sp.rows = rows;
    sp.ids = ids;
    sp.codes = codes;
    sp.sources = sources;
    sp.labels = labels;
    sp.o = *out;
    const int WL = W * L;
    sp.G = WL <= kWaveRowMax ? 64 : kStatsThreads;
    const int64_t lp_words = (int64_t)L * sp.C * sp.C;
    sp.lp_lds = labels && out->label_pairs && lp_words <= kLabelPairsLds ? (int)lp_words : 0;
    const int rpb = kStatsThreads / sp.G;
    const int64_t need = (rows + rpb - 1) / rpb;
    if (need > 2147483647LL) PN_FAIL(PN_ERR_ARG, "pn_walk_stats: too many rows for one launch");
    int64_t blocks = need < kMaxBlocks ? need : kMaxBlocks;
    // a workgroup counts in int32: it must see fewer than 2^31 entries
    if (blocks > 0 && ((need + blocks - 1) / blocks) * rpb * WL >= (1LL << 31)) blocks = need;
    if (int rc = pn::context_check_device(ctx)) return rc;

    if (!accumulate) {
        ZeroTabs z{};
        auto add = [&z](int64_t *ptr, int64_t count) {
            if (!ptr) return;
            z.ptr[z.k] = ptr;
            z.count[z.k++] = count;
        };
        add(out->step_code, (int64_t)L * L);
        add(out->label_pairs, lp_words);
        add(out->unlabeled, L);
        add(out->stay, L);
        add(out->back, L);
        add(out->distinct_hist, L + 1);
        add(out->visits, n);
        add(out->counters, 2);
        int64_t most = 0;
        for (int t = 0; t < z.k; t++) most = z.count[t] > most ? z.count[t] : most;
        if (z.k) {
            const int64_t zb = (most + kStatsThreads - 1) / kStatsThreads;
            hipLaunchKernelGGL(stats_zero_kernel, dim3((unsigned)(zb < 1024 ? zb : 1024)), dim3(kStatsThreads), 0, stream, z);
        }
    }
    if (blocks > 0) {
        const size_t lds = sizeof(int32_t) * ((size_t)L * L + 4 * L + 3 + sp.lp_lds + (size_t)rpb * (WL + (W + 1) / 2 + 2));
        hipLaunchKernelGGL(walk_stats_kernel, dim3((unsigned)blocks), dim3(kStatsThreads), lds, stream, sp);
    }
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int pn_path_multiplicity(pn_context *ctx, int32_t W, int32_t L, int64_t rows, const int32_t *ids, const uint8_t *codes,
                         float *mult, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_shape("pn_path_multiplicity", 1, W, L, rows, 0)) return rc;
    if (rows > 0 && (!ids || !mult)) PN_FAIL(PN_ERR_ARG, "pn_path_multiplicity: null ids or mult");
    if (int rc = pn::context_check_device(ctx)) return rc;
    if (rows == 0) return PN_OK;
    const int WL = W * L;
    const size_t lds = sizeof(int32_t) * (size_t)WL + (codes ? ((size_t)WL + 3) / 4 * 4 : 0);
    const int64_t blocks = rows < kMaxBlocks ? rows : kMaxBlocks;
    hipLaunchKernelGGL(path_mult_kernel, dim3((unsigned)blocks), dim3(kStatsThreads), lds, stream, W, L, rows, ids, codes, mult);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

}  // extern "C"
