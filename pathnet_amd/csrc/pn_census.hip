// pn_census.hip -- the synthetic-label generator (synthetic_data/gen_cora_syn.cpp, gen_citeseer_syn.cpp) on the device:
// for every node, the walks of k steps binned by the symbols of the nodes they visit, and the most frequent bin.
//   lists    every row (u, v) puts v into u's list and u into v's (:25-30): duplicates stay, a row u == u adds two
//            entries.  Both directions are written out as 2m (owner, entry) pairs, a stable radix sort by owner buckets
//            them (pn_sort.hip) and the bucket offsets are a binary search per node (pn_rows.h).  Order inside a list
//            does not matter: everything below is an integer sum.
//   census   the reference's DFS (:9-18) visits every walk; the same counts obey, level by level,
//                C_0[v] = [1],   C_j[u][b * B^(j-1) + r] = sum over the entries v of u's list with s[v] == b of C_(j-1)[v][r]
//            (the first step is the most significant digit).  One launch per level, in pull form: a node gathers the
//            rows of its list's entries and owns its output row, so there is no global atomic, no floating point, and
//            the counts are exact int64.  A wave owns a node and sums in LDS with integer adds.  With R = B^(j-1):
//              R < 64    a lane is (entry slot, r): 64 / R entries per step, kUnroll steps in flight
//              R >= 64   the lanes cover r, so the 8 R bytes of a row are read coalesced; kUnroll entries in flight
//            A list longer than kLongList entries is left to the end of the workgroup, whose four waves then share
//            it (their lanes add into one LDS row).  The last level's epilogue takes the argmax, lowest index on ties
//            (:37-40), and skips the table when the caller wants labels only.
// Gather-bound: level j reads (entries) * (4 + 1 + 8 R) bytes and writes 8 n B^j.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pathnet_hip.h"
#include "pn_internal.h"
#include "pn_rows.h"

namespace {

constexpr int kWaves = kThreads / 64;   // nodes per workgroup
constexpr int kLongList = 2048;         // entries; a longer list is shared by the workgroup's waves
constexpr int kUnroll = 4;              // list steps in flight per lane
constexpr int kMaxBins = 1024;          // B^k: four LDS rows of 8 KB per workgroup

typedef unsigned long long u64;

struct ListsWs {
    unsigned long long *status;
    int32_t *owner, *entry;         // [2m] both directions of every row
    int32_t *sorted;                // [2m] owners in bucket order
    void *sort_tmp;
    size_t sort_bytes;
};

size_t carve_lists(int64_t m, void *base, ListsWs *w) {
    Carver c{static_cast<char *>(base)};
    const size_t M2 = 2 * (size_t)(m > 0 ? m : 0);
    w->status = c.take<unsigned long long>(1);
    w->owner = c.take<int32_t>(M2);
    w->entry = c.take<int32_t>(M2);
    w->sorted = c.take<int32_t>(M2);
    w->sort_bytes = pn::sort_temp_reserve((int64_t)M2);
    w->sort_tmp = c.take<char>(w->sort_bytes);
    return c.at;
}

// B^k, or -1 when it exceeds kMaxBins
int bins_of(int B, int k) {
    int64_t x = 1;
    for (int i = 0; i < k; i++) {
        x *= B;
        if (x > kMaxBins) return -1;
    }
    return (int)x;
}

// row e -> (u, v) at e and (v, u) at m + e
__global__ __launch_bounds__(kThreads) void both_directions_kernel(int64_t m, const int32_t *__restrict__ u,
                                                                   const int32_t *__restrict__ v,
                                                                   int32_t *__restrict__ owner,
                                                                   int32_t *__restrict__ entry) {
    for (int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x; e < m; e += (int64_t)gridDim.x * kThreads) {
        const int32_t a = u[e], b = v[e];
        owner[e] = a;
        entry[e] = b;
        owner[m + e] = b;
        entry[m + e] = a;
    }
}

// row[b * R + r] += prev[v][r] for the entries v = adj[first], adj[first + stride], ... below `end`, this lane's r0,
// r0 + 64, ...; prev == nullptr is level 1, where every C_0 row is [1]
__device__ __forceinline__ void gather_list(const int32_t *__restrict__ adj, const uint8_t *__restrict__ sym,
                                            const int64_t *__restrict__ prev, int B, int R, int64_t first, int64_t end,
                                            int stride, int r0, u64 *row) {
    for (int64_t i = first; i < end; i += (int64_t)kUnroll * stride) {
        int32_t v[kUnroll];
        int b[kUnroll];
#pragma unroll
        for (int q = 0; q < kUnroll; q++) {
            const int64_t at = i + (int64_t)q * stride;
            v[q] = at < end ? adj[at] : -1;
        }
#pragma unroll
        for (int q = 0; q < kUnroll; q++) {
            b[q] = 0;
            if (v[q] >= 0) b[q] = sym ? min((int)sym[v[q]], B - 1) : (v[q] & 1);     // (no write leaves the row)
        }
        for (int r = r0; r < R; r += 64) {
            u64 x[kUnroll];
#pragma unroll
            for (int q = 0; q < kUnroll; q++) x[q] = v[q] < 0 ? 0 : prev ? (u64)prev[(int64_t)v[q] * R + r] : 1;
#pragma unroll
            for (int q = 0; q < kUnroll; q++)
                if (v[q] >= 0) atomicAdd(&row[b[q] * R + r], x[q]);
        }
    }
}

// one wave: the node's finished row to out (may be null) and its lowest-index argmax to labels (may be null)
__device__ __forceinline__ void finish_row(const u64 *row, int bins, int64_t node, int64_t *__restrict__ out,
                                           int64_t *__restrict__ labels, int lane) {
    long long best = -1;
    int arg = 0x7fffffff;
    for (int i = lane; i < bins; i += 64) {
        const long long c = (long long)row[i];
        if (out) out[node * bins + i] = c;
        if (c > best) {
            best = c;
            arg = i;
        }
    }
    if (!labels) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(arg, o, 64);
        if (ob > best || (ob == best && oa < arg)) {
            best = ob;
            arg = oa;
        }
    }
    if (lane == 0) labels[node] = arg;
}

// level j of the recurrence for the nodes [kWaves * blockIdx.x, +kWaves): prev = C_(j-1) rows of R = B^(j-1) counts
// (nullptr at level 1), out = C_j rows of B * R counts (nullptr: labels only).  Dynamic LDS: kWaves rows of B * R counts.
__global__ __launch_bounds__(kThreads) void census_level_kernel(int32_t n, const int64_t *__restrict__ off,
                                                                const int32_t *__restrict__ adj,
                                                                const uint8_t *__restrict__ sym, int B, int R,
                                                                const int64_t *__restrict__ prev,
                                                                int64_t *__restrict__ out,
                                                                int64_t *__restrict__ labels) {
    extern __shared__ u64 rows[];
    const int bins = B * R, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = blockIdx.x * (int64_t)kWaves;
    for (int i = threadIdx.x; i < kWaves * bins; i += kThreads) rows[i] = 0;
    // a lane's place in a step of its wave: (entry slot, r)
    const int per_step = R < 64 ? 64 / R : 1, slot = R < 64 ? lane / R : 0, r0 = R < 64 ? lane - slot * R : lane;
    const bool active = slot < per_step;
    const int64_t node = base + wave;
    int64_t begin = 0, end = 0;
    if (node < n) {
        begin = off[node];
        end = off[node + 1];
    }
    const bool own = node < n && end - begin <= kLongList;
    __syncthreads();
    if (own && active) gather_list(adj, sym, prev, B, R, begin + slot, end, per_step, r0, rows + wave * bins);
    __syncthreads();
    if (own) finish_row(rows + wave * bins, bins, node, out, labels, lane);
    // the long lists, one after the other, every wave on each; the row of such a node is still zero, and once its wave
    // has it nobody writes it again (every branch here is taken by the whole workgroup)
    for (int q = 0; q < kWaves; q++) {
        const int64_t nd = base + q;
        if (nd >= n) break;
        const int64_t b0 = off[nd], e0 = off[nd + 1];
        if (e0 - b0 <= kLongList) continue;
        if (active)
            gather_list(adj, sym, prev, B, R, b0 + wave * per_step + slot, e0, kWaves * per_step, r0, rows + q * bins);
        __syncthreads();
        if (wave == q) finish_row(rows + q * bins, bins, nd, out, labels, lane);
    }
}

}  // namespace

extern "C" {

int pn_census_lists_workspace_bytes(int32_t n, int64_t m, int64_t *bytes) {
    if (!bytes || n < 0 || m < 0) PN_FAIL(PN_ERR_ARG, "pn_census_lists_workspace_bytes: bad argument");
    ListsWs w;
    *bytes = (int64_t)(carve_lists(m, nullptr, &w) + 256);
    return PN_OK;
}

int pn_census_lists(pn_context *ctx, int32_t n, int64_t m, const int32_t *u, const int32_t *v, int64_t *off,
                    int32_t *adj, void *workspace, int64_t workspace_bytes, void *stream_) {
    if (n < 0 || m < 0 || !off || (m > 0 && (!u || !v || !adj))) PN_FAIL(PN_ERR_ARG, "pn_census_lists: bad argument");
    if (m >= (1LL << 30))
        PN_FAIL(PN_ERR_ARG, "pn_census_lists: the %lld list entries of %lld rows exceed the sort's int32 range",
                (long long)(2 * m), (long long)m);
    int64_t need = 0;
    pn_census_lists_workspace_bytes(n, m, &need);
    if (!workspace || workspace_bytes < need)
        PN_FAIL(PN_ERR_CAPACITY, "census list workspace holds %lld bytes, need %lld", (long long)workspace_bytes,
                (long long)need);
    if (int rc = pn::context_check_device(ctx)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ListsWs w;
    carve_lists(m, reinterpret_cast<void *>(((uintptr_t)workspace + 255) & ~(uintptr_t)255), &w);
    int64_t bad = -1;
    if (int rc = first_bad_row(n, m, u, v, w.status, stream, &bad)) return rc;
    if (bad >= 0) {
        int32_t a = 0, b = 0;
        if (int rc = read_row(u, v, bad, &a, &b, stream)) return rc;
        PN_FAIL(PN_ERR_ARG, "pair row %lld: node %d out of range", (long long)bad, (a < 0 || a >= n) ? a : b);
    }
    if (m > 0) {
        hipLaunchKernelGGL(both_directions_kernel, dim3(blocks_for(m)), dim3(kThreads), 0, stream, m, u, v, w.owner,
                           w.entry);
        if (int rc = pn::sort_pairs_i32(w.sort_tmp, w.sort_bytes, w.owner, w.sorted, w.entry, adj, 2 * m, key_bits_for(n),
                                        stream))
            return rc;
    }
    hipLaunchKernelGGL(bucket_off_kernel, dim3(blocks_for((int64_t)n + 1)), dim3(kThreads), 0, stream, n, 2 * m, w.sorted,
                       off);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int pn_pattern_census_workspace_bytes(int32_t n, int32_t num_symbols, int32_t walk_len, int64_t *bytes) {
    if (!bytes || n < 0) PN_FAIL(PN_ERR_ARG, "pn_pattern_census_workspace_bytes: bad argument");
    if (walk_len < 1) PN_FAIL(PN_ERR_ARG, "pattern census: walk_len %d, need at least 1", walk_len);
    if (num_symbols < 2 || num_symbols > 16) PN_FAIL(PN_ERR_ARG, "pattern census: %d symbols, need 2..16", num_symbols);
    if (bins_of(num_symbols, walk_len) < 0)
        PN_FAIL(PN_ERR_ARG, "pattern census: %d symbols over %d steps exceed %d patterns", num_symbols, walk_len, kMaxBins);
    // two level tables of n * B^(k-1) counts
    const int64_t table = walk_len > 1 ? (int64_t)n * bins_of(num_symbols, walk_len - 1) * 8 : 0;
    *bytes = 2 * ((table + 255) & ~(int64_t)255) + 256;
    return PN_OK;
}

int pn_pattern_census(pn_context *ctx, int32_t n, const int64_t *off, const int32_t *adj, const uint8_t *symbols,
                      int32_t num_symbols, int32_t walk_len, int64_t *counts, int64_t *labels, void *workspace,
                      int64_t workspace_bytes, void *stream_) {
    int64_t need = 0;
    if (int rc = pn_pattern_census_workspace_bytes(n, num_symbols, walk_len, &need)) return rc;
    if (!counts && !labels) PN_FAIL(PN_ERR_ARG, "pn_pattern_census: neither counts nor labels asked for");
    if (n > 0 && !off) PN_FAIL(PN_ERR_ARG, "pn_pattern_census: off is NULL");      // adj: NULL when the lists are empty
    if (walk_len > 1 && (!workspace || workspace_bytes < need))
        PN_FAIL(PN_ERR_CAPACITY, "pattern census workspace holds %lld bytes, need %lld", (long long)workspace_bytes,
                (long long)need);
    if (int rc = pn::context_check_device(ctx)) return rc;
    if (n == 0) return PN_OK;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    char *ws = reinterpret_cast<char *>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    int64_t *table[2] = {reinterpret_cast<int64_t *>(ws), reinterpret_cast<int64_t *>(ws + (need - 256) / 2)};
    const unsigned blocks = (unsigned)(((int64_t)n + kWaves - 1) / kWaves);
    const int64_t *prev = nullptr;
    int R = 1;
    for (int j = 1; j <= walk_len; j++, R *= num_symbols) {
        const bool last = j == walk_len;
        int64_t *out = last ? counts : table[j & 1];
        hipLaunchKernelGGL(census_level_kernel, dim3(blocks), dim3(kThreads),
                           (size_t)kWaves * num_symbols * R * sizeof(u64), stream, n, off, adj, symbols, (int)num_symbols, R,
                           prev, out, last ? labels : nullptr);
        prev = out;
    }
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

}  // extern "C"
