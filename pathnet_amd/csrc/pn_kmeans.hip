// pn_kmeans.hip -- k-means of fp32 rows by cosine or squared euclidean distance, and the scores of a grouping against labels
// (include/pathnet_hip.h carries the contract).  No [N, K] array is ever in memory, no floating-point atomic is used, and
// every sum has an order that depends on the shapes and the assignment alone: the same inputs give the same bits every run.
//
// The workspace holds the run's state: the prepared rows and the working centroids stacked as ONE array [N + K, D], so that
// logits_tile (pn_simtile.h) reads row tiles from the rows and column tiles from the centroids.
//
//   prepare_kernel   a wave per row: finiteness, fp64 norm (knn's order), liveness, the prepared row, q_r (ascending d)
//   offsets_kernel   a wave per centroid: h_c (the squares through LDS, one lane adds in ascending d), +inf for a centroid that
//                    is not live
//   assign_kernel    a workgroup per row tile of 64: walks the column tiles of 128 centroids, every lane keeps one (key, index)
//                    best for each of its 16 rows in registers; the lanes of a row meet by shuffles, the two column halves in LDS
//   blocksum_kernel  a wave per block of 256 rows: the rows through LDS, one lane adds in ascending order (row costs,
//                    k-means++ weights);
//                    up to 256 blocks the consuming kernel forms the sums itself
//   assign_finish    one workgroup: moved (integers), the block sums in ascending order, the done flag
//   seed_weight / seed_pick   one k-means++ round: min distances against the newest centroid, then the draw and the pick
//   keys / segments / partial / mean   the update: sort keys, (the stable sort,) segment offsets, chunk partials, the means
//   restart / keep_decide / keep_copy  the loop's bookkeeping: the best restart so far
//   scores_count / scores_finish       the contingency table by integer atomics, a one-workgroup finish in fp64
//
// Plain C++ and vector stores only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pn_internal.h"
#include "pn_kernels.h"
#include "pn_simtile.h"

namespace {

typedef unsigned long long u64;

constexpr int kMaxK = PN_KMEANS_MAX_K;
constexpr int kMaxD = 8192;
constexpr int kMaxIters = 65536;
constexpr int kMaxC = 4096;              // classes of pn_cluster_scores
constexpr int kBlk = 256;                // rows per block of the inertia and of the k-means++ prefix sums
constexpr int kChunk = 64;               // members per chunk of the update's segmented sums
constexpr double kDblMax = 1.7976931348623157e308;

static_assert(kMaxK == 1024, "h_c of a column tile, the scores' row sums and the key bits assume K <= 1024");

struct Header {            // the first 64 bytes of the workspace
    u64 dead;              // rows that are not live (prepare)
    int32_t done;          // the run's convergence flag
    int32_t iterations;    // assigns of the current restart that did work
    double inertia;        // of the current restart's last assign
    double best;           // the inertia held by the result
    int32_t take;          // keep_decide: the current restart replaces the result
    int32_t pad0;
    u64 pad[3];
};
static_assert(sizeof(Header) == 64, "the header is 64 bytes");

struct Ws {
    Header *head;
    float *Z;              // [N + K, D]: the prepared rows, then the working centroids
    int32_t *live;         // [N]
    double *q;             // [N]  sum_d x^2 (euclidean), 0 otherwise
    double *h;             // [K]  the centroids' offsets
    double *cost;          // [N]  row costs of the last assign / the weights of a k-means++ round
    double *mind;          // [N]  k-means++: the distance to the nearest centroid chosen so far
    double *bsum;          // [ceil(N / 256)]
    int32_t *tmoved;       // [ceil(N / 64)]  moved rows per row tile
    uint8_t *taken;        // [N]  k-means++: the row has been chosen
    int32_t *cur_label;    // [N]  the running restart's labels
    int64_t *cur_moved;    // [iters]
    int64_t *chosen;       // [K]
    int32_t *keys_in, *vals_in, *keys_out, *vals_out;      // [N] each
    int32_t *off;          // [K + 2]  off[c]: the first sorted position of cluster c; off[K]: of the dead rows
    int32_t *cstart;       // [K + 2]  cstart[c]: the first chunk of cluster c
    double *partial;       // [ceil(N / 64) + K, D]
    char *sort_tmp;
    size_t sort_bytes;
};

__host__ __device__ inline int64_t r8(int64_t b) { return (b + 7) & ~(int64_t)7; }

inline int64_t ws_layout(void *base, int64_t N, int32_t D, int32_t K, int32_t iters, Ws *w) {
    const uintptr_t p = (uintptr_t)base;        // (base may be null: the size query)
    const int64_t nb = (N + kBlk - 1) / kBlk, tiles = (N + kRT - 1) / kRT, chunks = (N + kChunk - 1) / kChunk + K;
    int64_t at = 0;
    auto take = [&](int64_t bytes) {
        char *q = (char *)(p + (uintptr_t)at);
        at += r8(bytes);
        return q;
    };
    w->head = (Header *)take(sizeof(Header));
    w->Z = (float *)take(4 * (N + K) * D);
    w->live = (int32_t *)take(4 * N);
    w->q = (double *)take(8 * N);
    w->h = (double *)take(8 * (int64_t)K);
    w->cost = (double *)take(8 * N);
    w->mind = (double *)take(8 * N);
    w->bsum = (double *)take(8 * nb);
    w->tmoved = (int32_t *)take(4 * tiles);
    w->taken = (uint8_t *)take(N);
    w->cur_label = (int32_t *)take(4 * N);
    w->cur_moved = (int64_t *)take(8 * (int64_t)iters);
    w->chosen = (int64_t *)take(8 * (int64_t)K);
    w->keys_in = (int32_t *)take(4 * N);
    w->vals_in = (int32_t *)take(4 * N);
    w->keys_out = (int32_t *)take(4 * N);
    w->vals_out = (int32_t *)take(4 * N);
    w->off = (int32_t *)take(4 * ((int64_t)K + 2));
    w->cstart = (int32_t *)take(4 * ((int64_t)K + 2));
    w->partial = (double *)take(8 * chunks * D);
    w->sort_bytes = pn::sort_temp_reserve(N);
    w->sort_tmp = take((int64_t)w->sort_bytes);
    return at;
}

inline int64_t ws_bytes(int64_t N, int32_t D, int32_t K, int32_t iters) {
    Ws w;
    return ws_layout(nullptr, N, D, K, iters, &w);
}

__device__ inline double wave_sum(double v) {       // a fixed butterfly: the same value, bit for bit, in all 64 lanes
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ inline bool finite_f(float v) { return fabsf(v) <= 3.4028234663852886e38f; }

__device__ inline int64_t label_at(const void *p, int32_t bits, int64_t r) {
    return bits == 64 ? ((const int64_t *)p)[r] : (int64_t)((const int32_t *)p)[r];
}
__device__ inline void label_put(void *p, int32_t bits, int64_t r, int64_t v) {
    if (bits == 64)
        ((int64_t *)p)[r] = v;
    else
        ((int32_t *)p)[r] = (int32_t)v;
}

// the cost of a live row whose best key is e
__device__ inline double row_cost(int32_t metric, double q, double e) {
    const double d = metric == PN_KMEANS_EUCLIDEAN ? q - 2.0 * e : 1.0 - e;
    return d > 0.0 ? d : 0.0;       // (a NaN cannot arise: e is never NaN, and q is finite)
}

// ---- prepare -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void kmeans_prepare_kernel(const float *__restrict__ X, int64_t ldx, int64_t N, int32_t D,
                                                                  int32_t metric, const uint8_t *__restrict__ valid, Ws w) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (r >= N) return;
    const float *x = X + r * ldx;
    double ss = 0.0;
    int fin = 1;
    for (int32_t d = lane; d < D; d += 64) {
        const float e = x[d];
        if (!finite_f(e)) fin = 0;
        ss += (double)e * (double)e;
    }
    fin = __all(fin);
    ss = wave_sum(fin ? ss : 0.0);
    const double nrm = sqrt(ss);
    const bool ok = fin && (metric == PN_KMEANS_EUCLIDEAN || (nrm > 0.0 && nrm <= kDblMax));
    const bool live = ok && (!valid || valid[r] != 0);
    float *z = w.Z + r * D;
    for (int32_t d = lane; d < D; d += 64)
        z[d] = !live ? 0.0f : metric == PN_KMEANS_EUCLIDEAN ? x[d] : (float)((double)x[d] / nrm);
    if (lane == 0) {
        double q = 0.0;
        if (live && metric == PN_KMEANS_EUCLIDEAN)
            for (int32_t d = 0; d < D; d++) q += (double)x[d] * (double)x[d];       // (the products are exact in fp64)
        w.q[r] = q;
        w.live[r] = live ? 1 : 0;
        if (!live) atomicAdd(&w.head->dead, 1ULL);
    }
}

// caller-supplied centroids into the stacked array
__global__ __launch_bounds__(kThreads) void kmeans_set_kernel(const float *__restrict__ C, int64_t ldc, int64_t N, int32_t D,
                                                              int32_t K, Ws w) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= (int64_t)K * D) return;
    const int64_t c = e / D;
    const int32_t d = (int32_t)(e % D);
    w.Z[(N + c) * D + d] = C[c * ldc + d];
}

// ---- the centroids' offsets ------------------------------------------------------------------------------------------------------
// a wave per centroid: 64 squares at a time through LDS, lane 0 adds them in ascending d
__global__ __launch_bounds__(kThreads) void kmeans_offsets_kernel(int64_t N, int32_t D, int32_t K, int32_t metric, Ws w,
                                                                  const int32_t *__restrict__ done) {
    __shared__ double sq[kThreads / 64][64];
    if (done && *done) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = blockIdx.x * (kThreads / 64) + wv;
    if (c >= K) return;         // (a whole wave; no workgroup barrier below)
    const float *m = w.Z + (N + c) * D;
    double ss = 0.0;
    int fin = 1;
    for (int32_t d0 = 0; d0 < D; d0 += 64) {
        const float e = d0 + lane < D ? m[d0 + lane] : 0.0f;
        if (!finite_f(e)) fin = 0;
        sq[wv][lane] = (double)e * (double)e;       // (exact)
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
            const int n = D - d0 < 64 ? D - d0 : 64;
            for (int i = 0; i < n; i++) ss += sq[wv][i];
        }
        __builtin_amdgcn_wave_barrier();
    }
    fin = __all(fin);
    const bool live = fin && (metric == PN_KMEANS_EUCLIDEAN || ss > 0.0);       // (a sum of at most 8192 fp32 squares is finite)
    if (lane == 0) w.h[c] = !live ? INFINITY : metric == PN_KMEANS_EUCLIDEAN ? 0.5 * ss : 0.0;
}

// ---- assign --------------------------------------------------------------------------------------------------------------------
__device__ inline bool better(double e, int32_t c, double best, int32_t arg) { return e > best || (e == best && c < arg); }

__global__ __launch_bounds__(kThreads) void kmeans_assign_kernel(int64_t N, int32_t D, int32_t K, int32_t metric, Ws w,
                                                                 const void *prev, void *label, int32_t bits,
                                                                 double *__restrict__ key, const int32_t *__restrict__ done) {
    __shared__ Stage st;
    __shared__ double hs[kCT];
    __shared__ double bk[2][kRT];
    __shared__ int32_t bi[2][kRT];
    if (done && *done) return;      // (the same in every thread of the grid)
    const int64_t n = N + K, r0 = (int64_t)blockIdx.x * kRT;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wr = wv >> 1, wc = wv & 1;
    double best[16];
    int32_t arg[16];
#pragma unroll
    for (int i = 0; i < 16; i++) {
        best[i] = -INFINITY;
        arg[i] = 0x7FFFFFFF;
    }
    for (int32_t c0 = 0; c0 < K; c0 += kCT) {
        __syncthreads();        // nobody reads the previous tile's offsets any more
        if (t < kCT) hs[t] = c0 + t < K ? w.h[c0 + t] : (double)INFINITY;
        f32x16 acc[2];
        logits_tile(w.Z, n, D, r0, N + c0, st, acc);        // (its barriers order the offsets before the reads below)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int cl = 64 * wc + 32 * j + (lane & 31);
            const int32_t c = c0 + cl;
            if (c < K) {
                const double hc = hs[cl];
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    float s = acc[j][i];
                    if (s != s) s = -INFINITY;
                    const double e = hc > kDblMax ? -(double)INFINITY : (double)s - hc;
                    if (better(e, c, best[i], arg[i])) {
                        best[i] = e;
                        arg[i] = c;
                    }
                }
            }
        }
    }
    // the 32 lanes that share a row, then the two column halves
#pragma unroll
    for (int i = 0; i < 16; i++) {
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) {
            const double ob = __shfl_xor(best[i], m, 64);
            const int32_t oa = __shfl_xor(arg[i], m, 64);
            if (better(ob, oa, best[i], arg[i])) {
                best[i] = ob;
                arg[i] = oa;
            }
        }
        if ((lane & 31) == 0) {
            const int rl = 32 * wr + 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3);
            bk[wc][rl] = best[i];
            bi[wc][rl] = arg[i];
        }
    }
    __syncthreads();
    if (t < kRT) {      // (wave 0)
        const int64_t row = r0 + t;
        int mv = 0;
        if (row < N) {
            double e = bk[0][t];
            int32_t a = bi[0][t];
            if (better(bk[1][t], bi[1][t], e, a)) {
                e = bk[1][t];
                a = bi[1][t];
            }
            const bool live = w.live[row] != 0;
            const int64_t lab = live ? (int64_t)a : -1;
            const int64_t pl = prev ? label_at(prev, bits, row) : lab + 1;      // (read before the label is written: they may alias)
            mv = live && pl != lab;
            if (label) label_put(label, bits, row, lab);
            if (key) key[row] = live ? e : -(double)INFINITY;
            w.cost[row] = live ? row_cost(metric, w.q[row], e) : 0.0;
        }
        const u64 b = __ballot(mv);
        if (t == 0) w.tmoved[blockIdx.x] = __popcll(b);
    }
}

// the sum of block b of 256 rows in ascending order, by one wave: the rows through LDS (buf: 256 doubles of this wave), lane 0 adds.
// The value is lane 0's.
__device__ inline double wave_block_sum(const double *__restrict__ cost, int64_t N, int64_t b, double *buf, int lane) {
    const int64_t r0 = b * kBlk;
    const int cnt = N - r0 < kBlk ? (int)(N - r0) : kBlk;
    for (int i = lane; i < cnt; i += 64) buf[i] = cost[r0 + i];
    __builtin_amdgcn_wave_barrier();
    double s = 0.0;
    if (lane == 0)
        for (int i = 0; i < cnt; i++) s += buf[i];
    __builtin_amdgcn_wave_barrier();
    return s;
}

// a wave per block of 256 rows.  With at most 256 blocks the kernel that consumes the sums forms them itself (local_block_sums)
__global__ __launch_bounds__(kThreads) void kmeans_blocksum_kernel(int64_t N, Ws w, const int32_t *__restrict__ done) {
    __shared__ double buf[kThreads / 64][kBlk];
    if (done && *done) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t b = (int64_t)blockIdx.x * (kThreads / 64) + wv, nb = (N + kBlk - 1) / kBlk;
    if (b >= nb) return;        // (a whole wave; no workgroup barrier below)
    const double s = wave_block_sum(w.cost, N, b, buf[wv], lane);
    if (lane == 0) w.bsum[b] = s;
}

// one workgroup of 256, at most 256 blocks: its four waves share the blocks; the same values as the kernel above.  buf: 4 x 256
// doubles.  All threads call; the sums are visible to all of them afterwards.
__device__ inline void local_block_sums(int64_t N, const Ws &w, double *buf) {
    const int64_t nb = (N + kBlk - 1) / kBlk;
    if (nb > kThreads) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int64_t b = wv; b < nb; b += kThreads / 64) {
        const double s = wave_block_sum(w.cost, N, b, buf + wv * kBlk, lane);
        if (lane == 0) w.bsum[b] = s;
    }
    __threadfence_block();
    __syncthreads();
}

constexpr int kStage = 4 * kBlk;        // doubles staged in LDS by the one-workgroup kernels

// thread 0 adds v[0 .. n) in ascending order, staged through LDS by the whole workgroup; the value is thread 0's.  All call.
__device__ inline double staged_sum(const double *__restrict__ v, int64_t n, double *stage) {
    double s = 0.0;
    for (int64_t i0 = 0; i0 < n; i0 += kStage) {
        const int m = n - i0 < kStage ? (int)(n - i0) : kStage;
        __syncthreads();
        for (int i = threadIdx.x; i < m; i += kThreads) stage[i] = v[i0 + i];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < m; i++) s += stage[i];
    }
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(kThreads) void kmeans_assign_finish_kernel(int64_t N, Ws w, int64_t *__restrict__ moved,
                                                                        double *__restrict__ inertia, int32_t *done,
                                                                        int32_t *iterations) {
    __shared__ double stage[kStage];
    __shared__ u64 mv;
    if (done && *done) return;
    const int64_t nb = (N + kBlk - 1) / kBlk, tiles = (N + kRT - 1) / kRT;
    if (threadIdx.x == 0) mv = 0;
    local_block_sums(N, w, stage);
    __syncthreads();
    u64 mine = 0;
    for (int64_t i = threadIdx.x; i < tiles; i += kThreads) mine += (u64)w.tmoved[i];
    if (mine) atomicAdd(&mv, mine);     // (integers: exact in any order)
    const double s = staged_sum(w.bsum, nb, stage);
    if (threadIdx.x == 0) {
        if (moved) moved[0] = (int64_t)mv;
        if (inertia) inertia[0] = s;
        if (iterations) iterations[0] += 1;
        if (done && mv == 0) *done = 1;
    }
}

// ---- k-means++ -----------------------------------------------------------------------------------------------------------------
// round j: the weight of every row -- 1 for a live row in round 0, afterwards the distance to the nearest centroid chosen so far
__global__ __launch_bounds__(kThreads) void kmeans_seed_weight_kernel(int64_t N, int32_t D, int32_t metric, Ws w, int32_t j) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (r >= N) return;
    const bool live = w.live[r] != 0;
    if (j == 0) {
        if (lane == 0) {
            w.mind[r] = INFINITY;
            w.taken[r] = 0;
            w.cost[r] = live ? 1.0 : 0.0;
        }
        return;
    }
    const int64_t c = w.chosen[j - 1];
    double wt = 0.0;
    if (live && c >= 0) {       // (the same in every lane)
        const float *a = w.Z + r * D, *b = w.Z + c * D;
        double dot = 0.0;
        for (int32_t d = lane; d < D; d += 64) dot += (double)a[d] * (double)b[d];      // (exact products)
        dot = wave_sum(dot);
        const double e = metric == PN_KMEANS_EUCLIDEAN ? dot - 0.5 * w.q[c] : dot;
        const double dist = row_cost(metric, w.q[r], e), old = w.mind[r];
        wt = dist < old ? dist : old;
        if (lane == 0) w.mind[r] = wt;
    }
    if (lane == 0) w.cost[r] = wt;
}

__global__ __launch_bounds__(kThreads) void kmeans_seed_pick_kernel(int64_t N, int32_t D, Ws w, u64 seed, int32_t restart,
                                                                    int32_t j) {
    __shared__ double stage[kStage];
    __shared__ int64_t pick_s, blk_s;
    __shared__ double tt_s, base_s;
    __shared__ int32_t low_free, low_live;
    const int t = threadIdx.x;
    const int64_t nb = (N + kBlk - 1) / kBlk;
    local_block_sums(N, w, stage);
    const double P = staged_sum(w.bsum, nb, stage);
    if (t == 0) {
        low_free = low_live = 0x7FFFFFFF;
        blk_s = -1;
        pick_s = -2;            // -2: the fallback order
        if (P > 0.0 && P <= kDblMax) {
            const uint4 x = pn::philox4(seed, ((u64)(uint32_t)restart << 32) | (u64)(uint32_t)j, PN_KMEANS_STREAM);
            const u64 r53 = ((u64)x.x | ((u64)x.y << 32)) >> 11;
            tt_s = ((double)r53 * 0x1p-53) * P;
            pick_s = -1;
        }
    }
    __syncthreads();
    if (pick_s == -1) {         // (the same in every thread)
        // the first block whose prefix passes t: the block sums once more, staged, one adder
        const double tt = tt_s;
        double B = 0.0;
        for (int64_t b0 = 0; b0 < nb; b0 += kStage) {
            const int m = nb - b0 < kStage ? (int)(nb - b0) : kStage;
            __syncthreads();
            if (blk_s >= 0) break;      // (written before the barrier, read by all after it)
            for (int i = t; i < m; i += kThreads) stage[i] = w.bsum[b0 + i];
            __syncthreads();
            if (t == 0)
                for (int i = 0; i < m; i++) {
                    const double B1 = B + stage[i];
                    if (B1 > tt) {
                        blk_s = b0 + i;
                        base_s = B;
                        break;
                    }
                    B = B1;
                }
        }
        __syncthreads();
        const int64_t b = blk_s;
        if (b >= 0) {           // the first row of that block whose prefix passes t
            const int64_t r0 = b * kBlk;
            const int cnt = N - r0 < kBlk ? (int)(N - r0) : kBlk;
            if (t < cnt) stage[t] = w.cost[r0 + t];
            __syncthreads();
            if (t == 0) {
                double p = 0.0;
                for (int i = 0; i < cnt; i++) {
                    p += stage[i];
                    if (base_s + p > tt) {
                        pick_s = r0 + i;
                        break;
                    }
                }
            }
        }
        // (t rounded up to P itself: the highest row with a weight)
        if (t == 0)
            for (int64_t r = N - 1; r >= 0 && pick_s < 0; r--)
                if (w.cost[r] > 0.0) pick_s = r;
    }
    __syncthreads();
    if (pick_s == -2) {     // the lowest live row not yet chosen; none: the lowest live row; none: no row
        int32_t f = 0x7FFFFFFF, l = 0x7FFFFFFF;
        for (int64_t r = N - 1 - t; r >= 0; r -= kThreads)
            if (w.live[r]) {
                l = (int32_t)r;
                if (!w.taken[r]) f = (int32_t)r;
            }
        if (l != 0x7FFFFFFF) atomicMin(&low_live, l);
        if (f != 0x7FFFFFFF) atomicMin(&low_free, f);
        __syncthreads();
        if (t == 0) pick_s = low_free != 0x7FFFFFFF ? low_free : low_live != 0x7FFFFFFF ? low_live : -1;
        __syncthreads();
    }
    const int64_t pick = pick_s;
    if (t == 0) {
        w.chosen[j] = pick;
        if (pick >= 0) w.taken[pick] = 1;
    }
    float *m = w.Z + (N + j) * D;
    for (int32_t d = t; d < D; d += kThreads) m[d] = pick >= 0 ? w.Z[pick * D + d] : 0.0f;
}

// ---- update --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void kmeans_keys_kernel(int64_t N, int32_t K, Ws w, const void *label, int32_t bits) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= N) return;
    const int64_t lab = label_at(label, bits, r);
    w.keys_in[r] = (w.live[r] != 0 && lab >= 0 && lab < K) ? (int32_t)lab : K;
    w.vals_in[r] = (int32_t)r;
}

__global__ __launch_bounds__(kThreads) void kmeans_segments_kernel(int64_t N, int32_t K, Ws w, int64_t *__restrict__ empty,
                                                                   const int32_t *__restrict__ done) {
    if (done && *done) return;
    for (int c = threadIdx.x; c <= K; c += kThreads) {      // the first sorted position whose key is >= c
        int64_t lo = 0, hi = N;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (w.keys_out[mid] < c)
                lo = mid + 1;
            else
                hi = mid;
        }
        w.off[c] = (int32_t)lo;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t at = 0;
        for (int c = 0; c < K; c++) {
            w.cstart[c] = at;
            at += (w.off[c + 1] - w.off[c] + kChunk - 1) / kChunk;
        }
        w.cstart[K] = at;
        if (empty) empty[0] = 0;
    }
}

// a workgroup per chunk of 64 members of one cluster: coordinate d of the chunk's sum, members in ascending order
__global__ __launch_bounds__(kThreads) void kmeans_partial_kernel(int32_t D, int32_t K, Ws w, const int32_t *__restrict__ done) {
    __shared__ int32_t rows[kChunk];
    if (done && *done) return;
    const int32_t b = blockIdx.x;
    if (b >= w.cstart[K]) return;
    int lo = 0, hi = K;         // cstart[lo] <= b < cstart[hi] throughout: the cluster that owns chunk b (it has members)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (w.cstart[mid] <= b)
            lo = mid;
        else
            hi = mid;
    }
    const int c = lo;
    const int32_t p0 = w.off[c] + (b - w.cstart[c]) * kChunk;
    const int32_t p1 = p0 + kChunk < w.off[c + 1] ? p0 + kChunk : w.off[c + 1];
    if ((int)threadIdx.x < p1 - p0) rows[threadIdx.x] = w.vals_out[p0 + threadIdx.x];
    __syncthreads();
    for (int32_t d = threadIdx.x; d < D; d += kThreads) {
        double s = 0.0;
        for (int p = 0; p < p1 - p0; p++) s += (double)w.Z[(int64_t)rows[p] * D + d];
        w.partial[(int64_t)b * D + d] = s;
    }
}

// a workgroup per cluster: the chunk partials in ascending order, the mean, the new centroid
__global__ __launch_bounds__(kThreads) void kmeans_mean_kernel(int64_t N, int32_t D, int32_t K, int32_t metric, Ws w,
                                                               int64_t *__restrict__ count, int64_t *__restrict__ empty,
                                                               const int32_t *__restrict__ done) {
    __shared__ double red[kThreads];
    if (done && *done) return;
    const int c = blockIdx.x, t = threadIdx.x;
    const int32_t cnt = w.off[c + 1] - w.off[c], c0 = w.cstart[c], nch = w.cstart[c + 1] - c0;
    if (t == 0 && count) count[c] = cnt;
    if (cnt == 0) {
        if (t == 0 && empty) atomicAdd((u64 *)empty, 1ULL);
        return;
    }
    float *m = w.Z + (N + c) * D;
    double sq = 0.0;
    for (int32_t d = t; d < D; d += kThreads) {
        double s = 0.0;
        for (int32_t i = 0; i < nch; i++) s += w.partial[(int64_t)(c0 + i) * D + d];
        const double mean = s / (double)cnt;
        if (metric == PN_KMEANS_EUCLIDEAN) {
            m[d] = (float)mean;
        } else {
            w.partial[(int64_t)c0 * D + d] = mean;      // (this workgroup owns the cluster's chunks)
            sq = __dadd_rn(sq, __dmul_rn(mean, mean));
        }
    }
    if (metric == PN_KMEANS_EUCLIDEAN) return;
    red[t] = sq;
    __syncthreads();
    for (int s = kThreads / 2; s >= 1; s >>= 1) {       // a fixed halving tree
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const double nrm = sqrt(red[0]);
    if (!(nrm > 0.0 && nrm <= kDblMax)) {       // the mean has no direction: the cluster keeps its centroid
        if (t == 0 && empty) atomicAdd((u64 *)empty, 1ULL);
        return;
    }
    for (int32_t d = t; d < D; d += kThreads) m[d] = (float)(w.partial[(int64_t)c0 * D + d] / nrm);
}

// ---- the loop's bookkeeping ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void kmeans_restart_kernel(Ws w, int32_t iters) {
    if (threadIdx.x == 0) {
        w.head->done = 0;
        w.head->iterations = 0;
        w.head->inertia = 0.0;
    }
    for (int32_t i = threadIdx.x; i < iters; i += kThreads) w.cur_moved[i] = -1;
}

__global__ __launch_bounds__(kThreads) void kmeans_keep_decide_kernel(Ws w, int32_t K, int32_t restart, int64_t *count,
                                                                      double *inertia, int32_t *iterations,
                                                                      int32_t *best_restart) {
    __shared__ int32_t take;
    if (threadIdx.x == 0) {
        const double cur = w.head->inertia, held = w.head->best;
        const bool cf = fabs(cur) <= kDblMax, hf = fabs(held) <= kDblMax;
        take = restart == 0 || (cf && (!hf || cur < held));
        w.head->take = take;
        if (take) {
            w.head->best = cur;
            if (inertia) inertia[0] = cur;
            if (iterations) iterations[0] = w.head->iterations;
            if (best_restart) best_restart[0] = restart;
        }
    }
    __syncthreads();
    if (take && count)
        for (int c = threadIdx.x; c < K; c += kThreads) count[c] = 0;
}

__global__ __launch_bounds__(kThreads) void kmeans_keep_copy_kernel(int64_t N, int32_t D, int32_t K, int32_t iters, Ws w,
                                                                    void *label, int32_t bits, float *__restrict__ centroid,
                                                                    int64_t *__restrict__ count, int64_t *__restrict__ moved) {
    if (!w.head->take) return;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < N) {
        const int32_t lab = w.cur_label[i];
        if (label) label_put(label, bits, i, lab);
        if (count && lab >= 0) atomicAdd((u64 *)&count[lab], 1ULL);
    }
    if (centroid && i < (int64_t)K * D) centroid[i] = w.Z[N * D + i];
    if (moved && i < iters) moved[i] = w.cur_moved[i];
}

// ---- scores --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void scores_count_kernel(const int64_t *__restrict__ pred, int32_t K,
                                                                const int64_t *__restrict__ truth, int32_t C, int64_t S,
                                                                int64_t *__restrict__ table, int64_t *__restrict__ skipped) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= S) return;
    const int64_t p = pred[i], y = truth[i];
    if (p >= 0 && p < K && y >= 0 && y < C)
        atomicAdd((u64 *)&table[p * C + y], 1ULL);
    else if (skipped)
        atomicAdd((u64 *)skipped, 1ULL);
}

__device__ inline int64_t choose2(int64_t v) { return v * (v - 1) / 2; }

__global__ __launch_bounds__(kThreads) void scores_finish_kernel(const int64_t *__restrict__ table, int32_t K, int32_t C,
                                                                 double *__restrict__ scores) {
    __shared__ u64 a[kMaxK];
    __shared__ u64 b[kMaxC];
    __shared__ double term[kThreads];
    __shared__ u64 pairs, maxes;
    const int t = threadIdx.x;
    const int64_t cells = (int64_t)K * C;
    for (int i = t; i < K; i += kThreads) a[i] = 0;
    for (int j = t; j < C; j += kThreads) b[j] = 0;
    if (t == 0) pairs = maxes = 0;
    __syncthreads();
    u64 my_pairs = 0;
    for (int64_t e = t; e < cells; e += kThreads) {
        const int64_t v = table[e];
        if (v > 0) {
            atomicAdd(&a[e / C], (u64)v);
            atomicAdd(&b[e % C], (u64)v);
            my_pairs += (u64)choose2(v);
        }
    }
    if (my_pairs) atomicAdd(&pairs, my_pairs);
    u64 my_max = 0;
    for (int i = t; i < K; i += kThreads) {
        int64_t mx = 0;
        for (int j = 0; j < C; j++) {
            const int64_t v = table[(int64_t)i * C + j];
            mx = v > mx ? v : mx;
        }
        my_max += (u64)mx;
    }
    if (my_max) atomicAdd(&maxes, my_max);
    __syncthreads();
    // the mutual information: the table's terms in row-major order, 256 at a time
    int64_t n = 0;
    for (int i = 0; i < K; i++) n += (int64_t)a[i];     // (every thread: integers)
    const double dn = (double)n;
    double mi = 0.0;
    for (int64_t e0 = 0; e0 < cells; e0 += kThreads) {
        const int64_t e = e0 + t;
        double v = 0.0;
        if (e < cells) {
            const int64_t nij = table[e];
            if (nij > 0) {
                const double x = (double)nij, ai = (double)(int64_t)a[e / C], bj = (double)(int64_t)b[e % C];
                v = __dmul_rn(x / dn, log(__dmul_rn(dn, x) / __dmul_rn(ai, bj)));
            }
        }
        __syncthreads();
        term[t] = v;
        __syncthreads();
        if (t == 0) {
            const int lim = cells - e0 < kThreads ? (int)(cells - e0) : kThreads;
            for (int i = 0; i < lim; i++) mi = __dadd_rn(mi, term[i]);
        }
    }
    if (t != 0) return;
    if (n == 0) {
        scores[0] = scores[1] = scores[2] = NAN;
        scores[3] = 0.0;
        return;
    }
    double hp = 0.0, ht = 0.0;
    int64_t A = 0, B = 0;
    for (int i = 0; i < K; i++) {
        const int64_t v = (int64_t)a[i];
        if (v > 0) {
            const double p = (double)v / dn;
            hp = __dadd_rn(hp, -__dmul_rn(p, log(p)));
            A += choose2(v);
        }
    }
    for (int j = 0; j < C; j++) {
        const int64_t v = (int64_t)b[j];
        if (v > 0) {
            const double p = (double)v / dn;
            ht = __dadd_rn(ht, -__dmul_rn(p, log(p)));
            B += choose2(v);
        }
    }
    const double hm = __dadd_rn(hp, ht) / 2.0;
    const double nmi = (hp == 0.0 && ht == 0.0) ? 1.0 : mi / hm;
    const double E = n > 1 ? __dmul_rn((double)A, (double)B) / (double)choose2(n) : 0.0;
    const double num = __dadd_rn((double)(int64_t)pairs, -E), den = __dadd_rn((double)(A + B) / 2.0, -E);
    scores[0] = nmi;
    scores[1] = den == 0.0 ? 1.0 : num / den;
    scores[2] = (double)(int64_t)maxes / dn;
    scores[3] = dn;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
int check_shape(const char *who, int64_t N, int32_t D, int32_t K, int32_t iters) {
    if (N < 0 || N >= 2147483648LL) PN_FAIL(PN_ERR_ARG, "%s: %lld rows, 0 <= N < 2^31", who, (long long)N);
    if (D < 1 || D > kMaxD) PN_FAIL(PN_ERR_ARG, "%s: %d columns, 1 .. %d", who, D, kMaxD);
    if (K < 1 || K > kMaxK) PN_FAIL(PN_ERR_ARG, "%s: %d clusters, 1 .. %d (PN_KMEANS_MAX_K)", who, K, kMaxK);
    if (iters < 0 || iters > kMaxIters) PN_FAIL(PN_ERR_ARG, "%s: %d iterations, 0 .. %d", who, iters, kMaxIters);
    return PN_OK;
}

int check_metric(const char *who, int32_t metric) {
    if (metric != PN_KMEANS_COSINE && metric != PN_KMEANS_EUCLIDEAN)
        PN_FAIL(PN_ERR_ARG, "%s: metric %d, PN_KMEANS_COSINE or PN_KMEANS_EUCLIDEAN", who, metric);
    return PN_OK;
}

int check_bits(const char *who, int32_t bits) {
    if (bits != 32 && bits != 64) PN_FAIL(PN_ERR_ARG, "%s: labels of %d bits, 32 or 64", who, bits);
    return PN_OK;
}

int check_ws(const char *who, int64_t N, int32_t D, int32_t K, int32_t iters, void *workspace, int64_t workspace_bytes, Ws *w) {
    if (!workspace) PN_FAIL(PN_ERR_ARG, "%s: null workspace", who);
    const int64_t need = ws_bytes(N, D, K, iters);
    if (workspace_bytes < need)
        PN_FAIL(PN_ERR_ARG, "%s: workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes, (long long)need);
    if ((uintptr_t)workspace & 7) PN_FAIL(PN_ERR_ARG, "%s: workspace not 8-byte aligned", who);
    ws_layout(workspace, N, D, K, iters, w);
    // (the sort may use what the caller gave beyond the formula)
    w->sort_bytes = (size_t)((char *)workspace + workspace_bytes - w->sort_tmp);
    return PN_OK;
}

inline unsigned grid_of(int64_t items, int per) { return (unsigned)((items + per - 1) / per); }

int key_bits_of(int32_t K) {
    int bits = 1;
    while ((1 << bits) <= K) bits++;
    return bits;
}

int do_prepare(const float *X, int64_t ldx, int64_t N, int32_t D, int32_t metric, const uint8_t *valid, const Ws &w,
               int64_t *counts, hipStream_t stream) {
    PN_CHECK_HIP(hipMemsetAsync(w.head, 0, sizeof(Header), stream));
    if (N > 0) hipLaunchKernelGGL(kmeans_prepare_kernel, dim3(grid_of(N, 4)), dim3(kThreads), 0, stream, X, ldx, N, D, metric, valid, w);
    if (counts) PN_CHECK_HIP(hipMemcpyAsync(counts, &w.head->dead, 8, hipMemcpyDeviceToDevice, stream));
    return PN_OK;
}

int do_seed(int64_t N, int32_t D, int32_t K, int32_t metric, u64 seed, int32_t restart, const Ws &w, hipStream_t stream) {
    const int64_t nb = (N + kBlk - 1) / kBlk;
    for (int32_t j = 0; j < K; j++) {
        if (N > 0) {
            hipLaunchKernelGGL(kmeans_seed_weight_kernel, dim3(grid_of(N, 4)), dim3(kThreads), 0, stream, N, D, metric, w, j);
            if (nb > kThreads)
                hipLaunchKernelGGL(kmeans_blocksum_kernel, dim3(grid_of(nb, 4)), dim3(kThreads), 0, stream, N, w, (const int32_t *)nullptr);
        }
        hipLaunchKernelGGL(kmeans_seed_pick_kernel, dim3(1), dim3(kThreads), 0, stream, N, D, w, seed, restart, j);
    }
    return PN_OK;
}

void do_assign(int64_t N, int32_t D, int32_t K, int32_t metric, const Ws &w, const void *prev, void *label, int32_t bits,
               double *key, int64_t *moved, double *inertia, int32_t *done, int32_t *iterations, hipStream_t stream) {
    const int64_t nb = (N + kBlk - 1) / kBlk;
    if (N > 0) {
        hipLaunchKernelGGL(kmeans_offsets_kernel, dim3(grid_of(K, 4)), dim3(kThreads), 0, stream, N, D, K, metric, w, (const int32_t *)done);
        hipLaunchKernelGGL(kmeans_assign_kernel, dim3(grid_of(N, kRT)), dim3(kThreads), 0, stream, N, D, K, metric, w, prev, label,
                           bits, key, (const int32_t *)done);
        if (nb > kThreads)
            hipLaunchKernelGGL(kmeans_blocksum_kernel, dim3(grid_of(nb, 4)), dim3(kThreads), 0, stream, N, w, (const int32_t *)done);
    }
    hipLaunchKernelGGL(kmeans_assign_finish_kernel, dim3(1), dim3(kThreads), 0, stream, N, w, moved, inertia, done, iterations);
}

int do_update(int64_t N, int32_t D, int32_t K, int32_t metric, const Ws &w, const void *label, int32_t bits, int64_t *count,
              int64_t *empty, const int32_t *done, hipStream_t stream) {
    if (N > 0) {
        hipLaunchKernelGGL(kmeans_keys_kernel, dim3(grid_of(N, kThreads)), dim3(kThreads), 0, stream, N, K, w, label, bits);
        // (the sort is the library's and cannot read the flag; what it writes is private to the workspace)
        if (int rc = pn::sort_pairs_i32(w.sort_tmp, w.sort_bytes, w.keys_in, w.keys_out, w.vals_in, w.vals_out, N, key_bits_of(K),
                                        stream))
            return rc;
    }
    hipLaunchKernelGGL(kmeans_segments_kernel, dim3(1), dim3(kThreads), 0, stream, N, K, w, empty, done);
    hipLaunchKernelGGL(kmeans_partial_kernel, dim3((unsigned)((N + kChunk - 1) / kChunk + K)), dim3(kThreads), 0, stream, D, K, w,
                       done);
    hipLaunchKernelGGL(kmeans_mean_kernel, dim3((unsigned)K), dim3(kThreads), 0, stream, N, D, K, metric, w, count, empty, done);
    return PN_OK;
}

}  // namespace

extern "C" {

int pn_kmeans_workspace_bytes(int64_t N, int32_t D, int32_t K, int32_t iters, int64_t *bytes) {
    if (!bytes) PN_FAIL(PN_ERR_ARG, "pn_kmeans_workspace_bytes: null result");
    if (int rc = check_shape("pn_kmeans_workspace_bytes", N, D, K, iters)) return rc;
    *bytes = ws_bytes(N, D, K, iters);
    return PN_OK;
}

int pn_kmeans_plan(int64_t N, int32_t D, int32_t K, int64_t out[6]) {
    if (!out) PN_FAIL(PN_ERR_ARG, "pn_kmeans_plan: null result");
    if (int rc = check_shape("pn_kmeans_plan", N, D, K, 0)) return rc;
    out[0] = (N + kRT - 1) / kRT;
    out[1] = kRT;
    out[2] = kCT;
    out[3] = kKC;
    out[4] = kChunk;
    out[5] = kBlk;
    return PN_OK;
}

int pn_kmeans_prepare(pn_context *ctx, const float *X, int64_t ldx, int64_t N, int32_t D, int32_t K, int32_t metric,
                      const uint8_t *valid, void *workspace, int64_t workspace_bytes, int64_t *counts, void *stream) {
    const char *who = "pn_kmeans_prepare";
    Ws w;
    if (int rc = check_shape(who, N, D, K, 0)) return rc;
    if (int rc = check_metric(who, metric)) return rc;
    if (N > 0 && !X) PN_FAIL(PN_ERR_ARG, "%s: null X", who);
    if (N > 0 && ldx < D) PN_FAIL(PN_ERR_ARG, "%s: row stride %lld below D = %d", who, (long long)ldx, D);
    if (int rc = check_ws(who, N, D, K, 0, workspace, workspace_bytes, &w)) return rc;
    if (int rc = pn::context_check_device(ctx)) return rc;
    if (int rc = do_prepare(X, ldx, N, D, metric, valid, w, counts, (hipStream_t)stream)) return rc;
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int pn_kmeans_set_centroids(pn_context *ctx, const float *centroid, int64_t ldc, int64_t N, int32_t D, int32_t K,
                            void *workspace, int64_t workspace_bytes, void *stream) {
    const char *who = "pn_kmeans_set_centroids";
    Ws w;
    if (int rc = check_shape(who, N, D, K, 0)) return rc;
    if (!centroid) PN_FAIL(PN_ERR_ARG, "%s: null centroids", who);
    if (ldc < D) PN_FAIL(PN_ERR_ARG, "%s: row stride %lld below D = %d", who, (long long)ldc, D);
    if (int rc = check_ws(who, N, D, K, 0, workspace, workspace_bytes, &w)) return rc;
    if (int rc = pn::context_check_device(ctx)) return rc;
    hipLaunchKernelGGL(kmeans_set_kernel, dim3(grid_of((int64_t)K * D, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, centroid,
                       ldc, N, D, K, w);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int pn_kmeans_seed(pn_context *ctx, int64_t N, int32_t D, int32_t K, int32_t metric, uint64_t seed, int32_t restart,
                   void *workspace, int64_t workspace_bytes, float *centroid, int64_t *chosen, void *stream_) {
    const char *who = "pn_kmeans_seed";
    hipStream_t stream = (hipStream_t)stream_;
    Ws w;
    if (int rc = check_shape(who, N, D, K, 0)) return rc;
    if (int rc = check_metric(who, metric)) return rc;
    if (restart < 0) PN_FAIL(PN_ERR_ARG, "%s: restart %d, >= 0", who, restart);
    if (int rc = check_ws(who, N, D, K, 0, workspace, workspace_bytes, &w)) return rc;
    if (int rc = pn::context_check_device(ctx)) return rc;
    if (int rc = do_seed(N, D, K, metric, seed, restart, w, stream)) return rc;
    if (centroid) PN_CHECK_HIP(hipMemcpyAsync(centroid, w.Z + N * D, 4 * (size_t)K * D, hipMemcpyDeviceToDevice, stream));
    if (chosen) PN_CHECK_HIP(hipMemcpyAsync(chosen, w.chosen, 8 * (size_t)K, hipMemcpyDeviceToDevice, stream));
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int pn_kmeans_assign(pn_context *ctx, int64_t N, int32_t D, int32_t K, int32_t metric, void *workspace, int64_t workspace_bytes,
                     const void *prev_label, int32_t label_bits, const pn_kmeans_assign_out *out, int32_t *done, void *stream) {
    const char *who = "pn_kmeans_assign";
    Ws w;
    if (int rc = check_shape(who, N, D, K, 0)) return rc;
    if (int rc = check_metric(who, metric)) return rc;
    if (int rc = check_bits(who, label_bits)) return rc;
    if (!out) PN_FAIL(PN_ERR_ARG, "%s: null output description", who);
    if (int rc = check_ws(who, N, D, K, 0, workspace, workspace_bytes, &w)) return rc;
    if (int rc = pn::context_check_device(ctx)) return rc;
    do_assign(N, D, K, metric, w, prev_label, out->label, label_bits, out->key, out->moved, out->inertia, done, out->iterations,
              (hipStream_t)stream);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int pn_kmeans_update(pn_context *ctx, int64_t N, int32_t D, int32_t K, int32_t metric, void *workspace, int64_t workspace_bytes,
                     const void *label, int32_t label_bits, float *centroid, int64_t *count, int64_t *empty, const int32_t *done,
                     void *stream_) {
    const char *who = "pn_kmeans_update";
    hipStream_t stream = (hipStream_t)stream_;
    Ws w;
    if (int rc = check_shape(who, N, D, K, 0)) return rc;
    if (int rc = check_metric(who, metric)) return rc;
    if (int rc = check_bits(who, label_bits)) return rc;
    if (N > 0 && !label) PN_FAIL(PN_ERR_ARG, "%s: null labels", who);
    if (int rc = check_ws(who, N, D, K, 0, workspace, workspace_bytes, &w)) return rc;
    if (int rc = pn::context_check_device(ctx)) return rc;
    if (int rc = do_update(N, D, K, metric, w, label, label_bits, count, empty, done, stream)) return rc;
    if (centroid) PN_CHECK_HIP(hipMemcpyAsync(centroid, w.Z + N * D, 4 * (size_t)K * D, hipMemcpyDeviceToDevice, stream));
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int pn_kmeans_run(pn_context *ctx, const float *X, int64_t ldx, int64_t N, int32_t D, int32_t K, int32_t metric,
                  const uint8_t *valid, const float *init, int64_t ld_init, int32_t iters, int32_t restarts, uint64_t seed,
                  void *workspace, int64_t workspace_bytes, int32_t label_bits, const pn_kmeans_out *out, void *stream_) {
    const char *who = "pn_kmeans_run";
    hipStream_t stream = (hipStream_t)stream_;
    Ws w;
    if (int rc = check_shape(who, N, D, K, iters)) return rc;
    if (int rc = check_metric(who, metric)) return rc;
    if (int rc = check_bits(who, label_bits)) return rc;
    if (iters < 1 || restarts < 1) PN_FAIL(PN_ERR_ARG, "%s: iters = %d, restarts = %d, at least 1 each", who, iters, restarts);
    if (init && restarts != 1) PN_FAIL(PN_ERR_ARG, "%s: %d restarts from the caller's centroids, 1 expected", who, restarts);
    if (init && ld_init < D) PN_FAIL(PN_ERR_ARG, "%s: row stride %lld of init below D = %d", who, (long long)ld_init, D);
    if (!out) PN_FAIL(PN_ERR_ARG, "%s: null output description", who);
    if (N > 0 && !X) PN_FAIL(PN_ERR_ARG, "%s: null X", who);
    if (N > 0 && ldx < D) PN_FAIL(PN_ERR_ARG, "%s: row stride %lld below D = %d", who, (long long)ldx, D);
    if (int rc = check_ws(who, N, D, K, iters, workspace, workspace_bytes, &w)) return rc;
    if (int rc = pn::context_check_device(ctx)) return rc;
    if (int rc = do_prepare(X, ldx, N, D, metric, valid, w, out->counts, stream)) return rc;
    for (int32_t rho = 0; rho < restarts; rho++) {
        hipLaunchKernelGGL(kmeans_restart_kernel, dim3(1), dim3(kThreads), 0, stream, w, iters);
        if (init) {
            hipLaunchKernelGGL(kmeans_set_kernel, dim3(grid_of((int64_t)K * D, kThreads)), dim3(kThreads), 0, stream, init, ld_init,
                               N, D, K, w);
        } else if (int rc = do_seed(N, D, K, metric, seed, rho, w, stream)) {
            return rc;
        }
        for (int32_t t = 0; t < iters; t++) {
            do_assign(N, D, K, metric, w, t == 0 ? nullptr : w.cur_label, w.cur_label, 32, nullptr, w.cur_moved + t,
                      &w.head->inertia, &w.head->done, &w.head->iterations, stream);
            if (t + 1 < iters)
                if (int rc = do_update(N, D, K, metric, w, w.cur_label, 32, nullptr, nullptr, &w.head->done, stream)) return rc;
        }
        hipLaunchKernelGGL(kmeans_keep_decide_kernel, dim3(1), dim3(kThreads), 0, stream, w, K, rho, out->count, out->inertia,
                           out->iterations, out->restart);
        int64_t items = N > (int64_t)K * D ? N : (int64_t)K * D;
        if (items < iters) items = iters;
        hipLaunchKernelGGL(kmeans_keep_copy_kernel, dim3(grid_of(items, kThreads)), dim3(kThreads), 0, stream, N, D, K, iters, w,
                           out->label, label_bits, out->centroid, out->count, out->moved);
    }
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int pn_cluster_scores(pn_context *ctx, const int64_t *pred, int32_t K, const int64_t *truth, int32_t C, int64_t S, int64_t *table,
                      int64_t *skipped, double *scores, void *stream_) {
    const char *who = "pn_cluster_scores";
    hipStream_t stream = (hipStream_t)stream_;
    if (S < 0 || S >= 2147483648LL) PN_FAIL(PN_ERR_ARG, "%s: %lld pairs, 0 <= S < 2^31", who, (long long)S);
    if (K < 1 || K > kMaxK) PN_FAIL(PN_ERR_ARG, "%s: %d clusters, 1 .. %d", who, K, kMaxK);
    if (C < 1 || C > kMaxC) PN_FAIL(PN_ERR_ARG, "%s: %d classes, 1 .. %d", who, C, kMaxC);
    if (!table) PN_FAIL(PN_ERR_ARG, "%s: null table", who);
    if (S > 0 && (!pred || !truth)) PN_FAIL(PN_ERR_ARG, "%s: null pred or truth", who);
    if (int rc = pn::context_check_device(ctx)) return rc;
    if (S > 0)
        hipLaunchKernelGGL(scores_count_kernel, dim3(grid_of(S, kThreads)), dim3(kThreads), 0, stream, pred, K, truth, C, S, table,
                           skipped);
    if (scores) hipLaunchKernelGGL(scores_finish_kernel, dim3(1), dim3(kThreads), 0, stream, (const int64_t *)table, K, C, scores);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

}  // extern "C"
