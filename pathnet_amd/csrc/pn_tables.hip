// pn_tables.hip -- the sampler's tables built on the device, bit-identical to the host builders of pn_host.cpp
// (pn_alias_build + pn_alias_pack + pn_node_ref_pack, pn_csr_build, pn_hops_dense), i.e. gen_merw.cpp:95-123 and
// AliasTable::init (:23-79).
//   bucketing   link() (:95-99) keeps every node's rows in file order: a stable radix sort of (u[e], e) is exactly that
//               order (pn_sort.hip's rocPRIM wrapper; the rocPRIM headers stay in that one translation unit).
//   alias       one lane per node runs the host's node_table: two FIFO queues (ring buffers of k entries over the node's
//               slice of the workspace), fp64 throughout, FP contraction off.  Every triple retires exactly one of the
//               node's k pending items (a pair step pops two and pushes one back, or emits the extra triple and pushes
//               none; a leftover is one triple), so a node's table holds k triples and off[] is the bucket prefix:
//               the host's count pass would count k for every node.
//   CSR         two stable sorts (by target, then by source) leave the pairs in (source, target) order; a unique flag,
//               a scan and a compaction drop the duplicates.
//   hops        one workgroup per source: a level-synchronous bounded BFS over the deduplicated out-lists, the source's
//               row of dis[] is the visited set (the labels do not depend on neighbour order or duplicates).
// Sort- and latency-bound (hubs run serially in one lane), not a streaming kernel.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/pathnet_hip.h"
#include "pn_internal.h"
#include "pn_rows.h"

#pragma clang fp contract(off)      // bit-identity with pn_host.cpp: no fused multiply-add anywhere in this file

namespace {

constexpr int kScanItems = 8;                               // items per thread of the unique-flag scan
constexpr int64_t kScanChunk = (int64_t)kThreads * kScanItems;

struct AliasWs {
    unsigned long long *status;     // first out-of-range row, ~0 when there is none
    int32_t *iota, *keys, *perm;    // sort values in, keys out, rows in bucketed order
    int32_t *hid, *lid;             // ring buffers of the heavy / light queues: node i uses [off[i], off[i+1])
    double *hmass, *lmass;
    void *sort_tmp;
    size_t sort_bytes;
};

struct CsrWs {
    unsigned long long *status;
    int32_t *k1, *v1;               // pairs sorted by target
    int32_t *s2, *d2;               // ... then stably by source: (source, target) order
    int32_t *pos;                   // [m + 1] exclusive scan of the unique flags
    int32_t *part;                  // [chunks + 1] per-chunk flag sums, scanned
    void *sort_tmp;
    size_t sort_bytes;
};

size_t carve_alias(int64_t m, void *base, AliasWs *w) {
    Carver c{static_cast<char *>(base)};
    const size_t M = (size_t)(m > 0 ? m : 0);
    w->status = c.take<unsigned long long>(1);
    w->iota = c.take<int32_t>(M);
    w->keys = c.take<int32_t>(M);
    w->perm = c.take<int32_t>(M);
    w->hid = c.take<int32_t>(M);
    w->lid = c.take<int32_t>(M);
    w->hmass = c.take<double>(M);
    w->lmass = c.take<double>(M);
    w->sort_bytes = pn::sort_temp_reserve(m);
    w->sort_tmp = c.take<char>(w->sort_bytes);
    return c.at;
}

size_t carve_csr(int64_t m, void *base, CsrWs *w) {
    Carver c{static_cast<char *>(base)};
    const size_t M = (size_t)(m > 0 ? m : 0);
    w->status = c.take<unsigned long long>(1);
    w->k1 = c.take<int32_t>(M);
    w->v1 = c.take<int32_t>(M);
    w->s2 = c.take<int32_t>(M);
    w->d2 = c.take<int32_t>(M);
    w->pos = c.take<int32_t>(M + 1);
    w->part = c.take<int32_t>((M + kScanChunk - 1) / kScanChunk + 1);
    w->sort_bytes = pn::sort_temp_reserve(m);
    w->sort_tmp = c.take<char>(w->sort_bytes);
    return c.at;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void iota_kernel(int64_t m, int32_t *__restrict__ out) {
    for (int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x; e < m; e += (int64_t)gridDim.x * kThreads)
        out[e] = (int32_t)e;
}

// draw_threshold of pn_host.cpp: the smallest draw r in [0, 2^31) with (1.0 * r / RAND_MAX) > s, or 2^31 (NaN included)
__device__ uint32_t draw_threshold(double s) {
    const double rmax = 2147483647.0;
    if (!(1.0 * 2147483647 / rmax > s)) return 2147483648u;
    uint32_t lo = 0, hi = 2147483647u;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (1.0 * (double)mid / rmax > s)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// FIFO queue of at most k items over a ring of k slots
struct Ring {
    int32_t *id;
    double *mass;
    int64_t k, head = 0, count = 0;
    __device__ void push(int32_t i, double ms) {
        int64_t at = head + count;
        if (at >= k) at -= k;
        id[at] = i;
        mass[at] = ms;
        count++;
    }
    __device__ void pop(int32_t &i, double &ms) {
        i = id[head];
        ms = mass[head];
        if (++head == k) head = 0;
        count--;
    }
};

// AliasTable::init of node i (pn_host.cpp node_table), one lane per node; writes its k triples {A, B, thr, 0} from
// off[i] on, the fp64 splits (S may be null) and node_ref[i] (may be null)
__global__ __launch_bounds__(kThreads) void alias_kernel(int32_t n, const int64_t *__restrict__ off,
                                                         const int32_t *__restrict__ perm, const int32_t *__restrict__ v,
                                                         const double *__restrict__ p, int32_t *hid, int32_t *lid,
                                                         double *hmass, double *lmass, int4 *__restrict__ triples,
                                                         double *__restrict__ S, uint32_t *__restrict__ node_ref) {
    const int64_t node = blockIdx.x * (int64_t)kThreads + threadIdx.x;
    if (node >= n) return;
    const int64_t base = off[node], k = off[node + 1] - base;
    if (node_ref) {
        node_ref[2 * node] = (uint32_t)base;
        node_ref[2 * node + 1] = (uint32_t)k;
    }
    if (k == 0) return;
    Ring heavy{hid + base, hmass + base, k}, light{lid + base, lmass + base, k};
    for (int64_t j = 0; j < k; j++) {
        const int32_t e = perm[base + j];
        const double mass = p[e] * (double)k;
        if (mass > 1.0)
            heavy.push(v[e], mass);
        else
            light.push(v[e], mass);
    }
    int64_t at = base;
    auto emit = [&](int32_t a, int32_t b, double s) {
        triples[at] = make_int4(a, b, (int32_t)draw_threshold(s), 0);
        if (S) S[at] = s;
        at++;
    };
    while (heavy.count > 0 && light.count > 0) {
        int32_t hv, lt;
        double hm, lm;
        heavy.pop(hv, hm);
        light.pop(lt, lm);
        emit(hv, lt, lm);
        const double rest = hm - (1.0 - lm);
        if (fabs(rest - 1.0) < 1e-5) {      // eps, gen_merw.cpp:5 and :48
            emit(hv, hv, rest);
            continue;
        }
        if (rest > 1.0)
            heavy.push(hv, rest);
        else
            light.push(hv, rest);
    }
    int32_t id;
    double ms;
    while (heavy.count > 0) {
        heavy.pop(id, ms);
        emit(id, id, 1.0);
    }
    while (light.count > 0) {
        light.pop(id, ms);
        emit(id, id, 1.0);
    }
}

// exclusive scan over the block's 256 threads; *total = the block's sum
__device__ int block_exclusive_scan(int x, int *lds, int *total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(inc, o, 64);
        if (lane >= o) inc += y;
    }
    if (lane == 63) lds[wv] = inc;
    __syncthreads();
    int before = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; w++) {
        const int t = lds[w];
        if (w < wv) before += t;
        sum += t;
    }
    __syncthreads();
    *total = sum;
    return before + inc - x;
}

// pair i of the (source, target)-sorted list is the first of its run
__device__ int unique_flag(const int32_t *__restrict__ s, const int32_t *__restrict__ d, int64_t i) {
    return i == 0 || s[i] != s[i - 1] || d[i] != d[i - 1];
}

// part[b] = number of unique pairs in chunk b
__global__ __launch_bounds__(kThreads) void flag_count_kernel(int64_t m, const int32_t *__restrict__ s,
                                                              const int32_t *__restrict__ d, int32_t *__restrict__ part) {
    __shared__ int lds[kThreads / 64];
    const int64_t i0 = blockIdx.x * kScanChunk + (int64_t)threadIdx.x * kScanItems;
    int c = 0;
    for (int j = 0; j < kScanItems; j++)
        if (i0 + j < m) c += unique_flag(s, d, i0 + j);
    int total;
    block_exclusive_scan(c, lds, &total);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// part[0, chunks) -> exclusive prefix; pos[m] = the total
__global__ __launch_bounds__(kThreads) void part_scan_kernel(int64_t chunks, int32_t *__restrict__ part, int64_t m,
                                                             int32_t *__restrict__ pos) {
    __shared__ int lds[kThreads / 64];
    int carry = 0;
    for (int64_t c = 0; c < chunks; c += kThreads) {
        const int64_t b = c + threadIdx.x;
        const int x = b < chunks ? part[b] : 0;
        int total;
        const int ex = block_exclusive_scan(x, lds, &total);
        if (b < chunks) part[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) pos[m] = carry;
}

// pos[i] = number of unique pairs before i
__global__ __launch_bounds__(kThreads) void flag_scan_kernel(int64_t m, const int32_t *__restrict__ s,
                                                             const int32_t *__restrict__ d,
                                                             const int32_t *__restrict__ part, int32_t *__restrict__ pos) {
    __shared__ int lds[kThreads / 64];
    const int64_t i0 = blockIdx.x * kScanChunk + (int64_t)threadIdx.x * kScanItems;
    int f[kScanItems], c = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; j++) {
        f[j] = i0 + j < m ? unique_flag(s, d, i0 + j) : 0;
        c += f[j];
    }
    int total;
    int at = part[blockIdx.x] + block_exclusive_scan(c, lds, &total);
#pragma unroll
    for (int j = 0; j < kScanItems; j++)
        if (i0 + j < m) {
            pos[i0 + j] = at;
            at += f[j];
        }
}

// off[x] = unique pairs with a source below x, x in [0, n]
__global__ __launch_bounds__(kThreads) void csr_off_kernel(int32_t n, int64_t m, const int32_t *__restrict__ s,
                                                           const int32_t *__restrict__ pos, int64_t *__restrict__ off) {
    for (int64_t x = blockIdx.x * (int64_t)kThreads + threadIdx.x; x <= n; x += (int64_t)gridDim.x * kThreads)
        off[x] = pos[lower_bound(s, m, (int32_t)x)];
}

__global__ __launch_bounds__(kThreads) void compact_kernel(int64_t m, const int32_t *__restrict__ s,
                                                           const int32_t *__restrict__ d, const int32_t *__restrict__ pos,
                                                           int32_t *__restrict__ adj) {
    for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < m; i += (int64_t)gridDim.x * kThreads)
        if (unique_flag(s, d, i)) adj[pos[i]] = d[i];
}

// one workgroup per source: row = dis[src][0, n); level l expands the nodes labelled l and labels their unvisited
// out-neighbours l + 1.  A lane that reads a label written in the same level sees l + 1, never l, so the level's
// frontier is exactly the nodes labelled before it began; two lanes writing the same label into one byte is benign.
__global__ __launch_bounds__(kThreads) void hops_kernel(int32_t n, const int64_t *__restrict__ off,
                                                        const int32_t *__restrict__ adj, int32_t seq_len, uint8_t *dis) {
    __shared__ int grew;
    const int32_t src = blockIdx.x;
    uint8_t *row = dis + (size_t)src * (size_t)n;
    for (int32_t y = threadIdx.x; y < n; y += kThreads) row[y] = y == src ? 1 : 0;
    __syncthreads();
    for (int32_t level = 1; level < seq_len; level++) {
        if (threadIdx.x == 0) grew = 0;
        __syncthreads();
        int any = 0;
        for (int32_t y = threadIdx.x; y < n; y += kThreads) {
            if (row[y] != level) continue;
            for (int64_t j = off[y]; j < off[y + 1]; j++) {
                const int32_t z = adj[j];
                if (row[z] == 0) {
                    row[z] = (uint8_t)(level + 1);
                    any = 1;
                }
            }
        }
        if (any) grew = 1;
        __syncthreads();
        if (!grew) break;
        __syncthreads();        // every lane has read grew before lane 0 clears it
    }
}

}  // namespace

extern "C" {

int pn_tables_workspace_bytes(int32_t n, int64_t m, int64_t *bytes) {
    if (!bytes || n < 0 || m < 0) PN_FAIL(PN_ERR_ARG, "pn_tables_workspace_bytes: bad argument");
    AliasWs a;
    CsrWs c;
    const size_t na = carve_alias(m, nullptr, &a), nc = carve_csr(m, nullptr, &c);
    *bytes = (int64_t)((na > nc ? na : nc) + 256);
    return PN_OK;
}

int pn_alias_build_device(int32_t n, int64_t m, const int32_t *u, const int32_t *v, const double *p, int64_t *off,
                          int32_t *triples, uint32_t *node_ref, double *S, int64_t cap, int64_t *total, void *workspace,
                          int64_t workspace_bytes, void *stream_) {
    if (n < 0 || m < 0 || !off || !total || (m > 0 && (!u || !v || !p)) || cap < 0)
        PN_FAIL(PN_ERR_ARG, "pn_alias_build_device: bad argument");
    if (m >= (1LL << 31)) PN_FAIL(PN_ERR_ARG, "pn_alias_build_device: %lld edge rows exceed the sort's int32 range", (long long)m);
    if (((uintptr_t)triples & 15) != 0) PN_FAIL(PN_ERR_ARG, "pn_alias_build_device: triples must be 16-byte aligned");
    int64_t need = 0;
    pn_tables_workspace_bytes(n, m, &need);
    if (!workspace || workspace_bytes < need)
        PN_FAIL(PN_ERR_CAPACITY, "tables workspace holds %lld bytes, need %lld", (long long)workspace_bytes, (long long)need);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    AliasWs w;
    carve_alias(m, reinterpret_cast<void *>(((uintptr_t)workspace + 255) & ~(uintptr_t)255), &w);
    int64_t bad = -1;
    if (int rc = first_bad_row(n, m, u, v, w.status, stream, &bad)) return rc;
    if (bad >= 0) {
        int32_t a = 0, b = 0;
        if (int rc = read_row(u, v, bad, &a, &b, stream)) return rc;
        if (a < 0 || a >= n) PN_FAIL(PN_ERR_ARG, "edge row %lld: source %d out of range", (long long)bad, a);
        PN_FAIL(PN_ERR_ARG, "edge row %lld: target %d out of range", (long long)bad, b);
    }
    *total = m;                     // k triples per node (see the top of this file)
    if (cap != 0 && cap < m)
        PN_FAIL(PN_ERR_CAPACITY, "alias buffers hold %lld triples, need %lld", (long long)cap, (long long)m);
    if (cap != 0 && m > 0 && !triples) PN_FAIL(PN_ERR_ARG, "pn_alias_build_device: triples is NULL");
    if (m > 0) {
        hipLaunchKernelGGL(iota_kernel, dim3(blocks_for(m)), dim3(kThreads), 0, stream, m, w.iota);
        if (int rc = pn::sort_pairs_i32(w.sort_tmp, w.sort_bytes, u, w.keys, w.iota, w.perm, m, key_bits_for(n), stream))
            return rc;
    }
    hipLaunchKernelGGL(bucket_off_kernel, dim3(blocks_for((int64_t)n + 1)), dim3(kThreads), 0, stream, n, m, w.keys, off);
    if (cap != 0 && n > 0)
        hipLaunchKernelGGL(alias_kernel, dim3((unsigned)(((int64_t)n + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                           stream, n, off, w.perm, v, p, w.hid, w.lid, w.hmass, w.lmass,
                           reinterpret_cast<int4 *>(triples), S, node_ref);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int pn_csr_build_device(int32_t n, int64_t m, const int32_t *u, const int32_t *v, int32_t reverse, int64_t *off,
                        int32_t *adj, int64_t cap, int64_t *count, void *workspace, int64_t workspace_bytes,
                        void *stream_) {
    if (n < 0 || m < 0 || !off || !count || (m > 0 && (!u || !v)) || cap < 0)
        PN_FAIL(PN_ERR_ARG, "pn_csr_build_device: bad argument");
    if (m >= (1LL << 31)) PN_FAIL(PN_ERR_ARG, "pn_csr_build_device: %lld edge rows exceed the sort's int32 range", (long long)m);
    int64_t need = 0;
    pn_tables_workspace_bytes(n, m, &need);
    if (!workspace || workspace_bytes < need)
        PN_FAIL(PN_ERR_CAPACITY, "tables workspace holds %lld bytes, need %lld", (long long)workspace_bytes, (long long)need);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    CsrWs w;
    carve_csr(m, reinterpret_cast<void *>(((uintptr_t)workspace + 255) & ~(uintptr_t)255), &w);
    int64_t bad = -1;
    if (int rc = first_bad_row(n, m, u, v, w.status, stream, &bad)) return rc;
    if (bad >= 0) PN_FAIL(PN_ERR_ARG, "edge row %lld out of range", (long long)bad);
    const int32_t *src = reverse ? v : u, *dst = reverse ? u : v;
    const int bits = key_bits_for(n);
    const int64_t chunks = (m + kScanChunk - 1) / kScanChunk;
    if (m > 0) {
        if (int rc = pn::sort_pairs_i32(w.sort_tmp, w.sort_bytes, dst, w.k1, src, w.v1, m, bits, stream)) return rc;
        if (int rc = pn::sort_pairs_i32(w.sort_tmp, w.sort_bytes, w.v1, w.s2, w.k1, w.d2, m, bits, stream)) return rc;
        hipLaunchKernelGGL(flag_count_kernel, dim3((unsigned)chunks), dim3(kThreads), 0, stream, m, w.s2, w.d2, w.part);
    }
    hipLaunchKernelGGL(part_scan_kernel, dim3(1), dim3(kThreads), 0, stream, chunks, w.part, m, w.pos);
    if (m > 0)
        hipLaunchKernelGGL(flag_scan_kernel, dim3((unsigned)chunks), dim3(kThreads), 0, stream, m, w.s2, w.d2, w.part,
                           w.pos);
    hipLaunchKernelGGL(csr_off_kernel, dim3(blocks_for((int64_t)n + 1)), dim3(kThreads), 0, stream, n, m, w.s2, w.pos, off);
    PN_CHECK_HIP(hipGetLastError());
    int32_t c = 0;
    PN_CHECK_HIP(hipMemcpyAsync(&c, w.pos + m, sizeof c, hipMemcpyDeviceToHost, stream));
    PN_CHECK_HIP(hipStreamSynchronize(stream));
    *count = c;
    if (cap != 0 && cap < c)
        PN_FAIL(PN_ERR_CAPACITY, "adjacency buffer holds %lld entries, need %lld", (long long)cap, (long long)c);
    if (cap != 0 && adj && m > 0)
        hipLaunchKernelGGL(compact_kernel, dim3(blocks_for(m)), dim3(kThreads), 0, stream, m, w.s2, w.d2, w.pos, adj);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int pn_hops_dense_device(int32_t n, const int64_t *off, const int32_t *adj, int32_t seq_len, uint8_t *dis,
                         void *stream_) {
    if (n < 0 || seq_len < 1 || seq_len > 254 || (n > 0 && (!off || !dis)))     // adj: NULL when the lists are empty
        PN_FAIL(PN_ERR_ARG, "pn_hops_dense_device: bad argument");
    if (n > 0)
        hipLaunchKernelGGL(hops_kernel, dim3((unsigned)n), dim3(kThreads), 0, static_cast<hipStream_t>(stream_), n, off,
                           adj, seq_len, dis);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

}  // extern "C"
