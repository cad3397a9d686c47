// pn_prob.hip -- transition probabilities of caller-supplied paths under the walker's own tables: pn_path_prob.
//
// The walker's step at a node cur with a table of k triples {A, B, thr} is exactly computable.  With r0 and r1 uniform on
// [0, 2^31) (glibc replay, and Philox word >> 1) it is  slot = r0 % k,  next = r1 >= thr[slot] ? A : B  -- the roll of
// pn_sampler.hip and of pn_bias.hip.  So the probability of cur -> x is an integer over 2^62:
//     base = 2^31 / k, rem = 2^31 % k,  c_s = base + (s < rem)                  the draws r0 that select slot s
//     cntA_s = max(0, 2^31 - thr_s),    cntB_s = min(thr_s, 2^31)               the draws r1 that select A / B
//     N(cur -> x) = sum_s c_s * (cntA_s * [A_s == x] + cntB_s * [B_s == x])     sum over x = 2^62: fits int64
// Uniform tables have A = B, so the same sum serves draws_per_step = 1.
//
// Second order (the biased walker's view): for transition t >= 1 with prev = ids[t-1] every candidate y of cur's table is
// of class 0 (y == prev), 1 (the hop source has the directed edge prev -> y: has_edge of pn_otf.h, the walker's own test)
// or 2; mass[c] is the sum of N(cur -> y) over the y of class c.  The kernel knows neither p nor q: the accept
// probabilities enter in pathnet_amd/pathprob.py, and one call serves every (p, q).
//
// path_prob_kernel: 16 lanes per transition, four transitions per wavefront, sixteen per workgroup.  The lanes of a group
// stride cur's triples, one 16-byte load each (256 contiguous bytes per round), keep int64 partial sums in registers and
// reduce them with __shfl_xor over 8 / 4 / 2 / 1; lane 0 of the group stores.  There is no floating point and every sum is
// a 64-bit integer add, so the result depends neither on the grouping nor on any order.  The workgroup strides over the
// transitions with 64-bit flat indices (rows * W * (L-1) may pass 2^31); the trip count of that loop is the same for every
// thread of the workgroup, so the shuffles always run with the whole wavefront.  Counters: lane -> wave -> LDS -> one
// atomic per workgroup and counter.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pn_internal.h"
#include "pn_otf.h"

namespace {

constexpr int kProbThreads = 256;
constexpr int kProbGroup = 16;                                  // lanes per transition
constexpr int kProbGroups = kProbThreads / kProbGroup;          // transitions per workgroup and turn
constexpr int kProbMaxBlocks = 2048;                            // 256 CUs x 8 resident workgroups
constexpr uint32_t kTwo31 = 0x80000000u;

typedef unsigned long long u64;

struct ProbParams {
    int32_t n;
    const int64_t *off;
    const int4 *triples;
    const uint2 *node_ref;      // [n] {first triple, count} or null: two words of off[]
    const uint8_t *dis;         // dense hop table, or null: adj_off / adj (second order only)
    const int64_t *adj_off;
    const int32_t *adj;
    int32_t L;
    int32_t second;
    int64_t total;              // transitions: rows * W * (L - 1)
    const int32_t *ids;
    pn_path_prob_out o;
};

__device__ __forceinline__ int64_t group_sum(int64_t v) {
#pragma unroll
    for (int o = kProbGroup / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// class of y for a walk that came from prev (in range): 0 return, 1 near, 2 far.  A table entry outside the graph (the
// library's builders make none) has no edge to it.
__device__ __forceinline__ int node_class(const ProbParams &p, int32_t prev, int32_t y) {
    if (y == prev) return 0;
    if ((uint32_t)y >= (uint32_t)p.n) return 2;
    return has_edge(p.dis, p.adj_off, p.adj, p.n, prev, y) ? 1 : 2;
}

__global__ __launch_bounds__(kProbThreads) void path_prob_kernel(ProbParams p) {
    __shared__ u64 s_cnt[3];
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int grp = threadIdx.x / kProbGroup, gl = threadIdx.x % kProbGroup;
    const int64_t T = p.L - 1;                   // transitions of a path
    u64 c_bad = 0, c_empty = 0, c_imp = 0;       // lane 0 of a group counts for its transitions
    for (int64_t base = (int64_t)blockIdx.x * kProbGroups; base < p.total; base += (int64_t)gridDim.x * kProbGroups) {
        const int64_t g = base + grp;
        const bool act = g < p.total;
        int64_t num = 0, m0 = 0, m1 = 0, m2 = 0;
        int32_t cur = -1, nxt = -1, prev = -1, len = 0;
        bool in_cur = false, in_nxt = false, classed = false;
        if (act) {
            const int64_t path = g / T;
            const int32_t t = (int32_t)(g - path * T);
            const int32_t *px = p.ids + path * p.L + t;
            cur = px[0];
            nxt = px[1];
            in_cur = (uint32_t)cur < (uint32_t)p.n;
            in_nxt = (uint32_t)nxt < (uint32_t)p.n;
            if (p.second && t >= 1) prev = px[-1];
            // classes exist for a transition inside the graph that has a prev inside the graph
            classed = in_cur && in_nxt && (uint32_t)prev < (uint32_t)p.n;
            if (in_cur && in_nxt) {
                int64_t o0;
                node_table(p.node_ref, p.off, cur, o0, len);
                if (len > 0) {
                    const uint32_t per = kTwo31 / (uint32_t)len, rem = kTwo31 % (uint32_t)len;
                    for (int32_t s = gl; s < len; s += kProbGroup) {
                        const int4 tr = p.triples[o0 + s];
                        const uint32_t thr = (uint32_t)tr.z;
                        const u64 c = (u64)per + ((uint32_t)s < rem ? 1u : 0u);
                        const int64_t nA = (int64_t)(c * (u64)(thr < kTwo31 ? kTwo31 - thr : 0u));
                        const int64_t nB = (int64_t)(c * (u64)(thr < kTwo31 ? thr : kTwo31));
                        num += (tr.x == nxt ? nA : 0) + (tr.y == nxt ? nB : 0);
                        if (classed) {
                            const int cA = node_class(p, prev, tr.x);
                            // (both candidates are the same node in uniform tables; a candidate no draw selects is not looked up)
                            const int cB = (tr.y == tr.x || nB == 0) ? cA : node_class(p, prev, tr.y);
                            m0 += (cA == 0 ? nA : 0) + (cB == 0 ? nB : 0);
                            m1 += (cA == 1 ? nA : 0) + (cB == 1 ? nB : 0);
                            m2 += (cA == 2 ? nA : 0) + (cB == 2 ? nB : 0);
                        }
                    }
                }
            }
        }
        num = group_sum(num);
        if (p.second) {
            m0 = group_sum(m0);
            m1 = group_sum(m1);
            m2 = group_sum(m2);
        }
        if (act && gl == 0) {
            if (p.o.num) p.o.num[g] = num;
            if (p.o.mass) {
                int64_t *m = p.o.mass + g * 3;
                m[0] = m0;
                m[1] = m1;
                m[2] = m2;
            }
            if (p.o.cls) p.o.cls[g] = (uint8_t)(classed ? node_class(p, prev, nxt) : 3);
            if (!in_cur || !in_nxt)
                c_bad += (in_cur ? 0 : 1) + (in_nxt ? 0 : 1);
            else if (len <= 0)
                c_empty++;
            else if (num == 0)
                c_imp++;
        }
    }
    if (p.o.counters) {
        c_bad = wave_sum(c_bad);
        c_empty = wave_sum(c_empty);
        c_imp = wave_sum(c_imp);
        if ((threadIdx.x & 63) == 0) {
            if (c_bad) atomicAdd(&s_cnt[0], c_bad);
            if (c_empty) atomicAdd(&s_cnt[1], c_empty);
            if (c_imp) atomicAdd(&s_cnt[2], c_imp);
        }
        __syncthreads();
        if (threadIdx.x < 3 && s_cnt[threadIdx.x])
            atomicAdd(reinterpret_cast<u64 *>(p.o.counters) + threadIdx.x, s_cnt[threadIdx.x]);
    }
}

int check_args(const char *who, const pn_sampler_tables *tb, int32_t W, int32_t L, int64_t rows, int32_t second_order) {
    if (!tb) PN_FAIL(PN_ERR_ARG, "%s: null tables", who);
    if (tb->n < 1 || W < 1 || L < 1 || rows < 0)
        PN_FAIL(PN_ERR_ARG, "%s: bad shape (n=%d W=%d L=%d rows=%lld)", who, tb->n, W, L, (long long)rows);
    if (rows > 0 && (int64_t)W * L > (1LL << 62) / rows)
        PN_FAIL(PN_ERR_ARG, "%s: %lld x %d x %d ids in one call", who, (long long)rows, W, L);
    if (second_order && !tb->dis && (!tb->adj_off || !tb->adj || !tb->radj_off || !tb->radj))
        PN_FAIL(PN_ERR_ARG, "%s: second order needs the walker's hop source: a dense hop table or the CSR lists", who);
    return PN_OK;
}

}  // namespace

extern "C" {

int pn_path_prob_workspace_bytes(const pn_sampler_tables *tb, int32_t W, int32_t L, int64_t rows, int32_t second_order,
                                 int64_t *bytes) {
    if (!bytes) PN_FAIL(PN_ERR_ARG, "pn_path_prob_workspace_bytes: null result");
    if (int rc = check_args("pn_path_prob_workspace_bytes", tb, W, L, rows, second_order)) return rc;
    *bytes = 0;         // a transition is summed in registers and the outputs are the caller's: nothing is kept in between
    return PN_OK;
}

int pn_path_prob(pn_context *ctx, const pn_sampler_tables *tb, int32_t W, int32_t L, int64_t rows, const int32_t *ids,
                 int32_t second_order, const pn_path_prob_out *out, void *workspace, int64_t workspace_bytes,
                 void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int64_t need = 0;
    if (int rc = check_args("pn_path_prob", tb, W, L, rows, second_order)) return rc;
    if (!out || (!ids && rows > 0)) PN_FAIL(PN_ERR_ARG, "pn_path_prob: null ids or output description");
    if ((!tb->off && !tb->node_ref) || !tb->triples) PN_FAIL(PN_ERR_ARG, "pn_path_prob: null table");
    if (tb->draws_per_step < 0 || tb->draws_per_step > 2)
        PN_FAIL(PN_ERR_ARG, "pn_path_prob: draws_per_step = %d (0, 1 or 2)", tb->draws_per_step);
    if (!second_order && (out->mass || out->cls)) PN_FAIL(PN_ERR_ARG, "pn_path_prob: mass / cls asked for without second_order");
    if (int rc = pn_path_prob_workspace_bytes(tb, W, L, rows, second_order, &need)) return rc;
    if (workspace_bytes < 0 || (need > 0 && (!workspace || workspace_bytes < need)))
        PN_FAIL(PN_ERR_ARG, "pn_path_prob: workspace holds %lld bytes, need %lld", (long long)(workspace ? workspace_bytes : 0),
                (long long)need);
    if (int rc = pn::context_check_device(ctx)) return rc;

    if (out->counters) PN_CHECK_HIP(hipMemsetAsync(out->counters, 0, 4 * sizeof(int64_t), stream));
    const int64_t total = rows * W * (int64_t)(L - 1);
    if (total == 0) return PN_OK;
    ProbParams pp{};
    pp.n = tb->n;
    pp.off = tb->off;
    pp.triples = reinterpret_cast<const int4 *>(tb->triples);
    pp.node_ref = reinterpret_cast<const uint2 *>(tb->node_ref);
    pp.dis = tb->dis;
    pp.adj_off = tb->adj_off;
    pp.adj = tb->adj;
    pp.L = L;
    pp.second = second_order ? 1 : 0;
    pp.total = total;
    pp.ids = ids;
    pp.o = *out;
    const int64_t want = (total + kProbGroups - 1) / kProbGroups;
    hipLaunchKernelGGL(path_prob_kernel, dim3((unsigned)(want < kProbMaxBlocks ? want : kProbMaxBlocks)), dim3(kProbThreads),
                       0, stream, pp);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

}  // extern "C"
