// pn_knn.hip -- exact k nearest neighbours of fp32 rows by cosine or dot product, tiled: no Sq x N array is ever in memory
// (include/pathnet_hip.h carries the contract), and the weighted vote over the neighbours' labels.
//
// The score of (query r, bank row c) is logits_tile's (pn_simtile.h): exact fp32 products, one k-ordered fma chain.  Every
// candidate becomes ONE 64-bit key,
//     key = orderable(score) << 32 | (0xFFFFFFFF - bank index),     orderable(b) = b < 0 ? ~bits : bits | 0x80000000
// so that "higher score first, lower index on equal bits" is one unsigned compare; -0.0 enters as +0.0 and a NaN (dot metric,
// overflowing products of both signs) as -inf.  No valid key is 0 (an index is below 2^31), so 0 is the empty slot.  The k best
// of a set of distinct keys do not depend on how the set is cut: a workgroup keeps the k best of its share of the column tiles
// and a merge kernel the k best of the partial lists -- the same bits for every split, launch width and run.
//
//   prep_kernel     a wave per row of Q and X: finiteness, fp64 norm, liveness, the row the MFMA reads (unit row or the row
//                   itself; zeros for a dead row) into the stacked Z [Sq + N, D]; the two dead counts by integer atomics
//   search_kernel   grid (row tiles of 64, splits).  Per column tile of 128: the scores, then per half of 64 columns the
//                   orderable scores go to LDS, and every wave folds 16 rows' 64 candidates into those rows' sorted lists in
//                   LDS (fold: drop what the list's last entry beats, rank the rest by counting, write each key to its rank)
//   merge_kernel    a wave per query: folds the `splits` partial lists in ascending split order, decodes index and score
//   vote_kernel     a wave per query: slot weights in fp64, added in ascending slot order into the wave's fp64 [C] in LDS
//
// No floating-point atomic; plain C++ and vector stores only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pn_internal.h"
#include "pn_simtile.h"

namespace {

typedef unsigned long long u64;

constexpr int kMaxK = PN_KNN_MAX_K;
constexpr int kMaxD = 8192;
constexpr int kMaxSplits = 1024;
constexpr int kMaxC = 4096;
constexpr int kHalf = kCT / 2;           // candidates per fold: one per lane
constexpr int64_t kTargetWG = 2 * 256;   // what splits = 0 aims at: two workgroups on each of the MI355X's 256 CUs
constexpr double kDblMax = 1.7976931348623157e308;

static_assert(kMaxK == 64 && kHalf == 64, "a list entry and a candidate per lane");
static_assert(sizeof(Stage) <= kRT * kHalf * 4, "the staged operands and the orderable scores share their LDS");

struct Header {            // the first 64 bytes of the workspace
    u64 dead_q, dead_x;
    u64 pad[6];
};

struct Ws {
    Header *head;
    u64 *part;             // [splits, Sq, k] keys, descending, 0 = empty
    float *Z;              // [Sq + N, D]: what the MFMA reads, the queries first
    int32_t *live;         // [Sq + N]
};

__host__ __device__ inline Ws ws_of(void *base, int64_t Sq, int64_t N, int32_t D, int32_t k, int32_t splits) {
    Ws w;
    char *p = (char *)base;
    w.head = (Header *)p;
    p += sizeof(Header);
    w.part = (u64 *)p;
    p += 8 * (int64_t)splits * Sq * k;
    w.Z = (float *)p;
    p += 4 * (Sq + N) * D;
    w.live = (int32_t *)p;
    return w;
}

inline int64_t ws_bytes(int64_t Sq, int64_t N, int32_t D, int32_t k, int32_t splits) {
    const int64_t b = (int64_t)sizeof(Header) + 8 * (int64_t)splits * Sq * k + 4 * (Sq + N) * D + 4 * (Sq + N);
    return (b + 7) & ~(int64_t)7;
}

// the splits a call runs with: the caller's, or enough for kTargetWG workgroups; never more than one per column tile
inline int32_t splits_of(int64_t Sq, int64_t N, int32_t splits_in) {
    if (Sq == 0 || N == 0) return 0;
    const int64_t rt = (Sq + kRT - 1) / kRT, ct = (N + kCT - 1) / kCT;
    int64_t s = splits_in > 0 ? splits_in : (kTargetWG + rt - 1) / rt;
    if (s > ct) s = ct;
    if (s > kMaxSplits) s = kMaxSplits;
    return (int32_t)s;
}

__device__ inline double wave_sum(double v) {       // a fixed butterfly: the same value, bit for bit, in all 64 lanes
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ inline bool finite_f(float v) { return fabsf(v) <= 3.4028234663852886e38f; }

__device__ inline uint32_t orderable(float s) {
    if (s != s) s = -INFINITY;
    if (s == 0.0f) s = 0.0f;
    const uint32_t b = __float_as_uint(s);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ inline float score_of(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o); }

// ---- prep ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void knn_prep_kernel(const float *__restrict__ Q, int64_t ldq, int64_t Sq,
                                                            const float *__restrict__ X, int64_t ldx, int64_t N, int32_t D,
                                                            int32_t k, int32_t splits, int32_t metric,
                                                            const uint8_t *__restrict__ bank_valid, void *ws) {
    const Ws w = ws_of(ws, Sq, N, D, k, splits);
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (r >= Sq + N) return;
    const bool query = r < Sq;
    const float *x = query ? Q + r * ldq : X + (r - Sq) * ldx;
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
    const bool ok = fin && (metric == PN_KNN_DOT || (nrm > 0.0 && nrm <= kDblMax));
    const bool wanted = query || !bank_valid || bank_valid[r - Sq] != 0;
    const bool live = wanted && ok;
    float *z = w.Z + r * D;
    for (int32_t d = lane; d < D; d += 64)
        z[d] = !live ? 0.0f : metric == PN_KNN_DOT ? x[d] : (float)((double)x[d] / nrm);
    if (lane == 0) {
        w.live[r] = live ? 1 : 0;
        if (wanted && !ok) atomicAdd(query ? &w.head->dead_q : &w.head->dead_x, 1ULL);
    }
}

// ---- fold: one wave, one candidate per lane, into a sorted list -------------------------------------------------------------------
// list: `cnt` distinct keys in descending order, room for k <= 64.  p: this lane's key, 0 = none, distinct from every other key.
// pk: 64 keys of scratch of this wave.  Afterwards the list holds the min(k, cnt + candidates) largest keys of the union, in
// descending order; returns that count.  A key's place is its rank, the number of keys above it, found by counting: the result
// depends on the set of keys alone.  All 64 lanes call this together.
__device__ inline int fold(u64 *list, int cnt, int k, u64 p, u64 *pk, int lane) {
    const u64 thr = cnt == k ? list[k - 1] : 0;
    const bool pass = p > thr;
    const u64 b = __ballot(pass);
    const int m = __popcll(b);
    if (m == 0) return cnt;
    if (pass) pk[__popcll(b & ((1ULL << lane) - 1))] = p;
    __builtin_amdgcn_wave_barrier();       // the passing keys are written before any lane reads them back
    const u64 mine = lane < cnt ? list[lane] : 0;
    int above_mine = 0, above_p = 0;       // passing keys above this lane's list entry / above its candidate
    for (int i = 0; i < m; i++) {
        const u64 q = pk[i];
        above_mine += q > mine;
        above_p += q > p;
    }
    int c = 0;                             // list entries above p: a prefix of the descending list
    for (int s = 64; s >= 1; s >>= 1)
        if (c + s <= cnt && list[c + s - 1] > p) c += s;
    __builtin_amdgcn_wave_barrier();       // every read of the old list is issued before the first write of the new one
    if (lane < cnt && lane + above_mine < k) list[lane + above_mine] = mine;
    if (pass && c + above_p < k) list[c + above_p] = p;
    __builtin_amdgcn_wave_barrier();
    return cnt + m < k ? cnt + m : k;
}

// ---- search --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void knn_search_kernel(int64_t Sq, int64_t N, int32_t D, int32_t k, int32_t splits,
                                                              const int64_t *__restrict__ exclude, void *ws) {
    __shared__ __attribute__((aligned(16))) uint32_t raw[kRT * kHalf];      // Stage, then the orderable scores [kRT][kHalf]
    __shared__ u64 list[kRT][kMaxK];
    __shared__ u64 pk[kThreads / 64][kHalf];
    __shared__ int32_t col_ok[kCT], row_ok[kRT], row_cnt[kRT], excl[kRT];
    Stage &st = *reinterpret_cast<Stage *>(raw);
    uint32_t(*T)[kHalf] = reinterpret_cast<uint32_t(*)[kHalf]>(raw);
    const Ws w = ws_of(ws, Sq, N, D, k, splits);
    const int64_t n = Sq + N, r0 = (int64_t)blockIdx.x * kRT;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wr = wv >> 1, wc = wv & 1;
    if (t < kRT) {
        const int64_t row = r0 + t;
        row_ok[t] = row < Sq && w.live[row] != 0;
        row_cnt[t] = 0;
        const int64_t e = (exclude && row < Sq) ? exclude[row] : -1;
        excl[t] = (e >= 0 && e < N) ? (int32_t)e : -1;
    }
    const int64_t tiles = (N + kCT - 1) / kCT;
    const int64_t tile0 = (int64_t)blockIdx.y * tiles / splits, tile1 = ((int64_t)blockIdx.y + 1) * tiles / splits;
    for (int64_t tile = tile0; tile < tile1; tile++) {
        const int64_t b0 = tile * kCT;          // the tile's first bank row
        __syncthreads();
        if (t < kCT) col_ok[t] = b0 + t < N ? w.live[Sq + b0 + t] : 0;
        f32x16 acc[2];
        logits_tile(w.Z, n, D, r0, Sq + b0, st, acc);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            __syncthreads();        // nobody reads the staged operands (h = 0) or the first half's scores (h = 1) any more
            if (wc == h) {
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const int rl = 32 * wr + 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3);
#pragma unroll
                    for (int j = 0; j < 2; j++) {
                        const int cl = 32 * j + (lane & 31);
                        const bool in = col_ok[kHalf * h + cl] != 0 && b0 + kHalf * h + cl != (int64_t)excl[rl];
                        T[rl][cl] = in ? orderable(acc[j][i]) : 0u;
                    }
                }
            }
            __syncthreads();
            for (int rr = 0; rr < kRT / 4; rr++) {
                const int row = (kRT / 4) * wv + rr;
                if (!row_ok[row]) continue;         // (the same in every lane)
                const uint32_t o = T[row][lane];
                const u64 key = o ? ((u64)o << 32 | (u64)(0xFFFFFFFFu - (uint32_t)(b0 + kHalf * h + lane))) : 0;
                const int cnt = fold(list[row], row_cnt[row], k, key, pk[wv], lane);
                if (lane == 0) row_cnt[row] = cnt;
            }
        }
    }
    __syncthreads();
    for (int rr = 0; rr < kRT / 4; rr++) {
        const int row = (kRT / 4) * wv + rr;
        const int64_t q = r0 + row;
        if (q < Sq && lane < k)
            w.part[((int64_t)blockIdx.y * Sq + q) * k + lane] = lane < row_cnt[row] ? list[row][lane] : 0;
    }
}

// ---- merge ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void knn_merge_kernel(int64_t Sq, int64_t N, int32_t D, int32_t k, int32_t splits,
                                                             const void *ws, int64_t *__restrict__ index,
                                                             float *__restrict__ score, int32_t *__restrict__ count,
                                                             int64_t *__restrict__ counts) {
    __shared__ u64 list[kThreads / 64][kMaxK];
    __shared__ u64 pk[kThreads / 64][kHalf];
    const Ws w = ws_of(const_cast<void *>(ws), Sq, N, D, k, splits);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0 && counts) {
        counts[0] = (int64_t)w.head->dead_q;
        counts[1] = (int64_t)w.head->dead_x;
    }
    const int64_t q = (int64_t)blockIdx.x * (kThreads / 64) + wv;
    if (q >= Sq) return;
    int cnt = 0;
    for (int32_t s = 0; s < splits; s++) {
        const u64 key = lane < k ? w.part[((int64_t)s * Sq + q) * k + lane] : 0;
        cnt = fold(list[wv], cnt, k, key, pk[wv], lane);
    }
    if (lane < k) {
        const u64 key = lane < cnt ? list[wv][lane] : 0;
        if (index) index[q * k + lane] = lane < cnt ? (int64_t)(0xFFFFFFFFu - (uint32_t)key) : -1;
        if (score) score[q * k + lane] = lane < cnt ? score_of((uint32_t)(key >> 32)) : -INFINITY;
    }
    if (lane == 0 && count) count[q] = cnt;
}

// ---- vote ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void knn_vote_kernel(const int64_t *__restrict__ index, const float *__restrict__ score,
                                                      const int32_t *__restrict__ count, int32_t k,
                                                      const int64_t *__restrict__ bank_labels, int64_t N, int32_t C, double T,
                                                      const int64_t *__restrict__ labels, double *__restrict__ prob,
                                                      int64_t *__restrict__ label, int64_t *__restrict__ confusion,
                                                      int64_t *__restrict__ skipped) {
    extern __shared__ double votes[];       // [C]
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    for (int c = lane; c < C; c += 64) votes[c] = 0.0;
    int cnt = count[q];
    cnt = cnt < 0 ? 0 : cnt > k ? k : cnt;
    // this lane's slot: its class (-1: does not vote) and weight
    int32_t cls = -1;
    double wt = 0.0;
    if (lane < cnt) {
        const int64_t idx = index[q * k + lane];
        if (idx >= 0 && idx < N) {
            const int64_t lab = bank_labels[idx];
            if (lab >= 0 && lab < C) {
                cls = (int32_t)lab;
                const float s0 = score[q * k], sj = score[q * k + lane];
                const double diff = sj == s0 ? 0.0 : (double)sj - (double)s0;
                wt = T > kDblMax ? 1.0 : exp(diff / T);
                if (!(wt >= 0.0)) wt = 0.0;         // (a NaN score)
            }
        }
    }
    __syncthreads();
    double total = 0.0;
    for (int j = 0; j < cnt; j++) {         // ascending slots, one adder
        const int32_t cj = __shfl(cls, j, 64);
        const double wj = __shfl(wt, j, 64);
        if (cj >= 0) {
            if (lane == 0) votes[cj] += wj;
            total += wj;
        }
    }
    __syncthreads();
    const bool any = total > 0.0;
    double best = -1.0;
    int32_t arg = -1;
    for (int c = lane; c < C; c += 64) {
        const double v = votes[c];
        if (prob) prob[q * C + c] = any ? v / total : 0.0;
        if (v > best) {
            best = v;
            arg = c;
        }
    }
    for (int m = 32; m >= 1; m >>= 1) {
        const double b2 = __shfl_xor(best, m, 64);
        const int32_t a2 = __shfl_xor(arg, m, 64);
        if (a2 >= 0 && (arg < 0 || b2 > best || (b2 == best && a2 < arg))) {
            best = b2;
            arg = a2;
        }
    }
    const int64_t out = any ? (int64_t)arg : -1;
    if (lane == 0) {
        if (label) label[q] = out;
        if (labels) {
            const int64_t y = labels[q];
            if (y >= 0 && y < C && out >= 0) {
                if (confusion) atomicAdd((u64 *)&confusion[y * C + out], 1ULL);
            } else if (skipped) {
                atomicAdd((u64 *)skipped, 1ULL);
            }
        }
    }
}

int check_shape(const char *who, int64_t Sq, int64_t N, int32_t D, int32_t k, int32_t splits) {
    if (Sq < 0 || Sq >= 2147483648LL) PN_FAIL(PN_ERR_ARG, "%s: %lld queries, 0 <= Sq < 2^31", who, (long long)Sq);
    if (N < 0 || N >= 2147483648LL) PN_FAIL(PN_ERR_ARG, "%s: %lld bank rows, 0 <= N < 2^31", who, (long long)N);
    if (D < 1 || D > kMaxD) PN_FAIL(PN_ERR_ARG, "%s: %d columns, 1 .. %d", who, D, kMaxD);
    if (k < 1 || k > kMaxK) PN_FAIL(PN_ERR_ARG, "%s: k = %d, 1 .. %d (PN_KNN_MAX_K)", who, k, kMaxK);
    if (splits < 0 || splits > kMaxSplits) PN_FAIL(PN_ERR_ARG, "%s: %d splits, 0 (the library chooses) .. %d", who, splits, kMaxSplits);
    return PN_OK;
}

}  // namespace

extern "C" {

int pn_knn_workspace_bytes(int64_t Sq, int64_t N, int32_t D, int32_t k, int32_t splits, int64_t *bytes) {
    if (!bytes) PN_FAIL(PN_ERR_ARG, "pn_knn_workspace_bytes: null result");
    if (int rc = check_shape("pn_knn_workspace_bytes", Sq, N, D, k, splits)) return rc;
    *bytes = ws_bytes(Sq, N, D, k, splits_of(Sq, N, splits));
    return PN_OK;
}

int pn_knn_plan(int64_t Sq, int64_t N, int32_t D, int32_t k, int32_t splits_in, int64_t out[4]) {
    if (!out) PN_FAIL(PN_ERR_ARG, "pn_knn_plan: null result");
    if (int rc = check_shape("pn_knn_plan", Sq, N, D, k, splits_in)) return rc;
    const int32_t splits = splits_of(Sq, N, splits_in);
    out[0] = splits;
    out[1] = (Sq + kRT - 1) / kRT * splits;
    out[2] = kRT;
    out[3] = kCT;
    return PN_OK;
}

int pn_knn_search(pn_context *ctx, const float *Q, int64_t ldq, int64_t Sq, const float *X, int64_t ldx, int64_t N, int32_t D,
                  int32_t k, int32_t metric, const uint8_t *bank_valid, const int64_t *exclude, int32_t splits_in,
                  void *workspace, int64_t workspace_bytes, const pn_knn_out *out, void *stream_) {
    const char *who = "pn_knn_search";
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_shape(who, Sq, N, D, k, splits_in)) return rc;
    if (metric != PN_KNN_COSINE && metric != PN_KNN_DOT) PN_FAIL(PN_ERR_ARG, "%s: metric %d, PN_KNN_COSINE or PN_KNN_DOT", who, metric);
    if (!out) PN_FAIL(PN_ERR_ARG, "%s: null output description", who);
    if ((Sq > 0 && !Q) || (N > 0 && !X) || !workspace) PN_FAIL(PN_ERR_ARG, "%s: null Q, X or workspace", who);
    if ((Sq > 0 && ldq < D) || (N > 0 && ldx < D))
        PN_FAIL(PN_ERR_ARG, "%s: row strides %lld / %lld below D = %d", who, (long long)ldq, (long long)ldx, D);
    const int32_t splits = splits_of(Sq, N, splits_in);
    if (workspace_bytes < ws_bytes(Sq, N, D, k, splits))
        PN_FAIL(PN_ERR_ARG, "%s: workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes,
                (long long)ws_bytes(Sq, N, D, k, splits));
    if ((uintptr_t)workspace & 7) PN_FAIL(PN_ERR_ARG, "%s: workspace not 8-byte aligned", who);
    if (int rc = pn::context_check_device(ctx)) return rc;
    const dim3 block(kThreads);
    PN_CHECK_HIP(hipMemsetAsync(workspace, 0, sizeof(Header), stream));
    if (Sq + N > 0)
        hipLaunchKernelGGL(knn_prep_kernel, dim3((unsigned)((Sq + N + 3) / 4)), block, 0, stream, Q, ldq, Sq, X, ldx, N, D, k,
                           splits, metric, bank_valid, workspace);
    if (splits > 0)
        hipLaunchKernelGGL(knn_search_kernel, dim3((unsigned)((Sq + kRT - 1) / kRT), (unsigned)splits), block, 0, stream, Sq, N, D,
                           k, splits, exclude, workspace);
    // (with Sq == 0 one workgroup writes counts; with N == 0 there are no partial lists and every slot is empty)
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)(Sq > 0 ? (Sq + 3) / 4 : 1)), block, 0, stream, Sq, N, D, k, splits,
                       (const void *)workspace, out->index, out->score, out->count, out->counts);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int pn_knn_vote(pn_context *ctx, const int64_t *index, const float *score, const int32_t *count, int64_t Sq, int32_t k,
                const int64_t *bank_labels, int64_t N, int32_t C, double T, const int64_t *labels, double *prob, int64_t *label,
                int64_t *confusion, int64_t *skipped, void *stream_) {
    const char *who = "pn_knn_vote";
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_shape(who, Sq, N, 1, k, 0)) return rc;
    if (C < 1 || C > kMaxC) PN_FAIL(PN_ERR_ARG, "%s: %d classes, 1 .. %d", who, C, kMaxC);
    if (!(T > 0.0)) PN_FAIL(PN_ERR_ARG, "%s: temperature %g, > 0 (+inf: the plain majority vote)", who, T);
    if (Sq > 0 && (!index || !score || !count)) PN_FAIL(PN_ERR_ARG, "%s: null index, score or count", who);
    if (Sq > 0 && N > 0 && !bank_labels) PN_FAIL(PN_ERR_ARG, "%s: null bank labels", who);
    if ((confusion || skipped) && !labels) PN_FAIL(PN_ERR_ARG, "%s: confusion / skipped without the queries' labels", who);
    if (int rc = pn::context_check_device(ctx)) return rc;
    if (Sq == 0) return PN_OK;
    hipLaunchKernelGGL(knn_vote_kernel, dim3((unsigned)Sq), dim3(64), (size_t)C * sizeof(double), stream, index, score, count, k,
                       bank_labels, N, C, T, labels, prob, label, confusion, skipped);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

}  // extern "C"
