// pn_bias.hip -- second-order (return / in-out biased) random walks: pn_sample_paths_biased.
//
// The plain walker (pn_sampler.hip) is first-order: the next node depends on the current one alone.  Here step t >= 1 of
// a walk at node cur that came from prev has the target distribution
//     P(x)  ~  P_table(cur -> x) * a(prev, x),    a = 1/p  x == prev                       (class 0, return)
//                                                     1    the directed edge prev -> x exists (class 1, near)
//                                                     1/q  otherwise                          (class 2, far)
// (node2vec's return parameter p and in-out parameter q; p = inf is a non-backtracking walk).  Step 0 has no prev and
// is the plain table step.
//
// The walk is realised by rejection sampling with the walker's own alias / uniform table as the proposal:
//   thresholds  T_c = floor(2^32 * w_c / max(w)),  w = {1/p, 1, 1/q}  (pn_bias_thresholds: fp64, host, one place)
//   trial j of a walk (j counts over ALL its steps) reads Philox4x32-10 block j of the walk's subsequence
//     (subsequence = the plain walker's global walk index, key = the seed):
//     word 0 >> 1  slot draw (% table length);  word 1 >> 1  alias probability draw (>= thr ? A : B);
//     word 2       accept draw: the proposal is taken iff word 2 < T_class;  word 3 unused.
//   A step takes at most PN_BIAS_MAX_TRIALS trials: its 64th proposal is taken whatever the accept draw says, and the
//   step is counted in `exhausted` -- the way out of a leaf under p = inf, and the bound of every lane's loop.
//   A walk of length L makes L - 1 transitions and draws nothing after its last node.
//
// bias_walk_kernel: one walk per lane, ONE flat trial loop.  A lane carries its own step counter t: a lane whose
// proposal is accepted goes on to its next step in the next iteration while its neighbours still reject, so a wave
// runs max-over-lanes(total trials) iterations, not sum-over-steps(max-over-lanes(trials)).  The loop ends after at
// most (L - 1) * 64 iterations.  "Is prev -> x an edge" is one byte of the dense hop table (dis[prev][x] == 2) or a
// binary search of prev's sorted out-list (on-the-fly mode); both hop sources give the same walks.
//
// Distance codes: with the dense table the walker gathers the byte dis[source][x] itself, by pn_path_codes' formula.
// On the fly the codes come from pn_path_codes' own launch over the ids just written (same stream) -- the ball search
// exists once, in pn_codes.hip / pn_otf.h.
#include <hip/hip_runtime.h>

#include <cmath>

#include "pn_internal.h"
#include "pn_otf.h"

namespace {

constexpr int kBiasThreads = 256;

struct BiasParams {
    int32_t n;
    const int64_t *off;
    const int4 *triples;
    const uint2 *node_ref;      // [n] {first triple, count} or null: two words of off[]
    const uint8_t *dis;         // dense hop table, or null: adj_off / adj
    const int64_t *adj_off;
    const int32_t *adj;
    int32_t W, L;
    uint64_t seed;
    int64_t epoch_begin, epoch_count;
    int32_t node_begin, node_count;
    int32_t *ids;
    uint8_t *codes;             // written in dense mode only
    int32_t *status;
    const pn_step_state *dyn;
    const int32_t *node_list;
    unsigned long long thr[3];  // accept thresholds of the classes, in [0, 2^32]
    unsigned long long *exhausted;
};

// Philox4x32-10 (Random123): block `ctr` of subsequence `sub` under key `seed` -- what rocRAND's generator returns as
// the ctr-th group of four words after rocrand_init(seed, sub, 0)
__device__ __forceinline__ uint4 philox_block(uint64_t seed, uint64_t sub, uint32_t ctr) {
    uint32_t c0 = ctr, c1 = 0, c2 = (uint32_t)sub, c3 = (uint32_t)(sub >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}

// pn_path_codes' dense formula: 0 = unreached, else hops + 1
__device__ __forceinline__ uint8_t dense_code(const BiasParams &p, int32_t st, int32_t x) {
    const int b = p.dis[(size_t)st * (size_t)p.n + (size_t)x];
    return (uint8_t)((b == 0 || b > p.L) ? p.L - 1 : b - 1);
}

__global__ __launch_bounds__(kBiasThreads) void bias_walk_kernel(BiasParams p) {
    __shared__ unsigned s_exhausted;
    if (threadIdx.x == 0) s_exhausted = 0;
    __syncthreads();
    const int64_t per_epoch = (int64_t)p.node_count * p.W;
    const int64_t total = per_epoch * p.epoch_count;
    const int64_t g = (int64_t)blockIdx.x * kBiasThreads + threadIdx.x;
    unsigned n_exhausted = 0;
    if (g < total) {
        const int64_t e_l = g / per_epoch;
        const int64_t rem = g - e_l * per_epoch;
        const int32_t st_i = (int32_t)(rem / p.W);
        // (a listed source node outside the graph is clamped, as in the plain walker)
        const int32_t st = p.node_list ? min(max(p.node_list[st_i], 0), p.n - 1) : p.node_begin + st_i;
        const int32_t wi = (int32_t)(rem % p.W);
        const int64_t epoch_begin = p.dyn ? p.dyn->epoch : p.epoch_begin;
        const uint64_t seed = p.dyn ? p.dyn->seed : p.seed;
        const uint64_t walk = ((uint64_t)(epoch_begin + e_l) * (uint64_t)p.n + (uint64_t)st) * (uint64_t)p.W + wi;
        const bool flat_far = p.thr[1] == p.thr[2];       // q = 1: near and far weigh the same, no edge test
        int32_t *out_ids = p.ids + g * p.L;
        uint8_t *out_codes = p.dis ? p.codes + g * p.L : nullptr;

        const int32_t last = p.L - 1;        // transitions of the walk
        int32_t x = st, prev = st;
        int32_t t = 0;                       // transitions made: x is path node t
        int32_t k = 0;                       // trials of the current step so far
        uint32_t j = 0;                      // trials of the walk so far = the next Philox block
        uint8_t code = 0;                    // of x (dense mode)
        out_ids[0] = st;
        if (out_codes) out_codes[0] = code = dense_code(p, st, st);
        int64_t o0 = 0;
        int32_t len = 0;
        if (last > 0) node_table(p.node_ref, p.off, x, o0, len);
        // every iteration is one trial of this lane's current step; at most 64 per step
        for (int32_t it = 0; it < last * PN_BIAS_MAX_TRIALS && t < last; it++) {
            if (len <= 0) {
                if (p.status) atomicExch(p.status, PN_ERR_EMPTY_TABLE);
                for (int32_t f = t + 1; f <= last; f++) {        // the rest of the path repeats this node
                    out_ids[f] = x;
                    if (out_codes) out_codes[f] = code;
                }
                break;
            }
            const uint4 w = philox_block(seed, walk, j++);
            const int4 tr = p.triples[o0 + (int64_t)((w.x >> 1) % (uint32_t)len)];
            const int32_t cand = ((w.y >> 1) >= (uint32_t)tr.z) ? tr.x : tr.y;
            bool take = t == 0;
            k++;
            if (!take) {
                unsigned long long T;
                if (cand == prev)
                    T = p.thr[0];
                else if (flat_far)
                    T = p.thr[1];
                else
                    T = has_edge(p.dis, p.adj_off, p.adj, p.n, prev, cand) ? p.thr[1] : p.thr[2];
                take = (unsigned long long)w.z < T;
                if (k == PN_BIAS_MAX_TRIALS) {
                    take = true;
                    n_exhausted++;
                }
            }
            if (take) {
                prev = x;
                x = cand;
                t++;
                k = 0;
                out_ids[t] = x;
                if (out_codes) out_codes[t] = code = dense_code(p, st, x);
                if (t < last) node_table(p.node_ref, p.off, x, o0, len);
            }
        }
    }
    // steps that hit the trial cap: lane -> wave -> workgroup (LDS) -> one atomic per workgroup
    if (p.exhausted) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n_exhausted += __shfl_xor(n_exhausted, o);
        if ((threadIdx.x & 63) == 0 && n_exhausted) atomicAdd(&s_exhausted, n_exhausted);
        __syncthreads();
        if (threadIdx.x == 0 && s_exhausted) atomicAdd(p.exhausted, (unsigned long long)s_exhausted);
    }
}

int check_args(const char *who, const pn_sampler_tables *tb, int32_t W, int32_t L, int64_t epoch_count, int32_t node_count,
               bool *otf) {
    if (!tb) PN_FAIL(PN_ERR_ARG, "%s: null tables", who);
    if (tb->n < 1 || W < 1 || L < 1 || epoch_count < 0 || node_count < 0)
        PN_FAIL(PN_ERR_ARG, "%s: bad shape (n=%d W=%d L=%d epochs=%lld nodes=%d)", who, tb->n, W, L, (long long)epoch_count,
                node_count);
    if (L > 254) PN_FAIL(PN_ERR_ARG, "%s: L = %d (a code is one byte and the dense table holds hops + 1)", who, L);
    *otf = tb->dis == nullptr;
    if (*otf && (!tb->adj_off || !tb->adj || !tb->radj_off || !tb->radj))
        PN_FAIL(PN_ERR_ARG, "%s: neither a dense hop table nor the CSR lists for on-the-fly hop codes", who);
    if (*otf && (tb->n >= (1 << 28) || L > 8))
        PN_FAIL(PN_ERR_ARG, "on-the-fly hop codes support n < 2^28 and L <= 8 (n=%d L=%d)", tb->n, L);
    if (epoch_count * (int64_t)node_count > 2147483647LL)
        PN_FAIL(PN_ERR_ARG, "%s: %lld x %d rows in one call (at most 2^31 - 1)", who, (long long)epoch_count, node_count);
    return PN_OK;
}

}  // namespace

extern "C" {

int pn_bias_thresholds(double p, double q, uint64_t thr[3]) {
    if (!thr) PN_FAIL(PN_ERR_ARG, "pn_bias_thresholds: null result");
    if (!(p > 0.0) || !(q > 0.0))       // (also refuses NaN)
        PN_FAIL(PN_ERR_ARG, "pn_bias_thresholds: p and q must be > 0 (+inf allowed), got p=%g q=%g", p, q);
    const double w[3] = {std::isinf(p) ? 0.0 : 1.0 / p, 1.0, std::isinf(q) ? 0.0 : 1.0 / q};
    double m = w[0];
    for (int c = 1; c < 3; c++) m = w[c] > m ? w[c] : m;
    for (int c = 0; c < 3; c++) thr[c] = (uint64_t)std::floor(std::ldexp(w[c] / m, 32));    // the largest: exactly 2^32
    return PN_OK;
}

int pn_sample_paths_biased_workspace_bytes(const pn_sampler_tables *tb, int32_t W, int32_t L, int64_t epoch_count,
                                           int32_t node_count, int64_t *bytes) {
    bool otf;
    if (!bytes) PN_FAIL(PN_ERR_ARG, "pn_sample_paths_biased_workspace_bytes: null result");
    if (int rc = check_args("pn_sample_paths_biased_workspace_bytes", tb, W, L, epoch_count, node_count, &otf)) return rc;
    *bytes = 0;         // dense: the walker reads the code bytes itself
    if (otf) return pn_path_codes_workspace_bytes(tb, W, L, (int32_t)(epoch_count * node_count), bytes);
    return PN_OK;
}

int pn_sample_paths_biased(pn_context *ctx, const pn_sampler_tables *tb, int32_t W, int32_t L, uint64_t seed,
                           int64_t epoch_begin, int64_t epoch_count, int32_t node_begin, int32_t node_count, double p,
                           double q, int32_t *ids, uint8_t *codes, int64_t *exhausted, void *workspace,
                           int64_t workspace_bytes, int32_t *status_flag, const pn_step_state *step_state,
                           const int32_t *node_list, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    bool otf;
    if (int rc = check_args("pn_sample_paths_biased", tb, W, L, epoch_count, node_count, &otf)) return rc;
    if (!tb->off || !tb->triples || !ids || !codes) PN_FAIL(PN_ERR_ARG, "pn_sample_paths_biased: null table or output");
    if (tb->draws_per_step < 0 || tb->draws_per_step > 2)
        PN_FAIL(PN_ERR_ARG, "pn_sample_paths_biased: draws_per_step = %d (0, 1 or 2)", tb->draws_per_step);
    BiasParams bp{};
    {
        uint64_t thr[3];
        if (int rc = pn_bias_thresholds(p, q, thr)) return rc;
        for (int c = 0; c < 3; c++) bp.thr[c] = thr[c];
    }
    if (node_list) node_begin = 0;
    if (epoch_begin < 0 || node_begin < 0 || (!node_list && (int64_t)node_begin + node_count > tb->n))
        PN_FAIL(PN_ERR_ARG, "pn_sample_paths_biased: bad window (n=%d epoch %lld nodes [%d,+%d))", tb->n,
                (long long)epoch_begin, node_begin, node_count);
    int64_t need = 0;
    if (int rc = pn_sample_paths_biased_workspace_bytes(tb, W, L, epoch_count, node_count, &need)) return rc;
    if (need > 0 && (!workspace || workspace_bytes < need))
        PN_FAIL(PN_ERR_ARG, "pn_sample_paths_biased: workspace holds %lld bytes, need %lld",
                (long long)(workspace ? workspace_bytes : 0), (long long)need);
    const int64_t total = epoch_count * node_count * W;
    if (total / kBiasThreads + 1 > 2147483647LL) PN_FAIL(PN_ERR_ARG, "pn_sample_paths_biased: window too large for one launch");
    if (int rc = pn::context_check_device(ctx)) return rc;

    if (exhausted) PN_CHECK_HIP(hipMemsetAsync(exhausted, 0, sizeof(int64_t), stream));
    if (total == 0) return PN_OK;
    bp.n = tb->n;
    bp.off = tb->off;
    bp.triples = reinterpret_cast<const int4 *>(tb->triples);
    bp.node_ref = reinterpret_cast<const uint2 *>(tb->node_ref);
    bp.dis = tb->dis;
    bp.adj_off = tb->adj_off;
    bp.adj = tb->adj;
    bp.W = W;
    bp.L = L;
    bp.seed = seed;
    bp.epoch_begin = epoch_begin;
    bp.epoch_count = epoch_count;
    bp.node_begin = node_begin;
    bp.node_count = node_count;
    bp.ids = ids;
    bp.codes = codes;
    bp.status = status_flag;
    bp.dyn = step_state;
    bp.node_list = node_list;
    bp.exhausted = reinterpret_cast<unsigned long long *>(exhausted);
    {
        pn::StageTimer tm(ctx, pn::ST_SAMPLER_WALK, stream);
        hipLaunchKernelGGL(bias_walk_kernel, dim3((unsigned)((total + kBiasThreads - 1) / kBiasThreads)), dim3(kBiasThreads),
                           0, stream, bp);
    }
    PN_CHECK_HIP(hipGetLastError());
    if (otf)        // the row's source is its first id: every walk of a row starts there
        return pn_path_codes(ctx, tb, W, L, (int32_t)(epoch_count * node_count), ids, nullptr, codes, nullptr, workspace,
                             workspace_bytes, stream);
    return PN_OK;
}

}  // extern "C"
