// pn_ensemble.hip -- ensemble prediction over resampled paths (pn_ensemble_add / pn_ensemble_add_scaled / pn_ensemble_finish).
//
// A PathNet prediction depends on the W paths the sampler drew for the node.  K independent draws give K logit rows per
// node; this file averages their class probabilities where they are and says how much the draws disagree.
//
//   ensemble_add_kernel<G, false>  logits [R, S, C] fp32 -> the caller's state (psum, hsum, votes, count, bad).  ONE group of G
//                              threads owns state row index[s] and takes its R samples in ascending r, so no floating-point
//                              atomic exists and one [R, S, C] call leaves the bits of R calls of [1, S, C].
//   ensemble_add_kernel<G, true>  the same body with exp((x_c - m) / tau), tau read on the device (pn_ensemble_add_scaled)
//   ensemble_finish_kernel<G>  state -> prob, label, vote_label, confidence, entropy, mutual_info, agreement, and with a
//                              target the confusion matrix (integer atomics: exact, order-free).
//
// Work split (pn_ensemble_route) and the order of a sum over classes: pn_group.h.  G depends on C alone, and so does the
// order -- not on S, R, rows, the grid or the index.  All arithmetic after the fp32 -> fp64 conversion of a logit is fp64.
// Plain C++ and vector stores only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pn_group.h"
#include "pn_internal.h"

namespace {

using namespace pn::group;        // kThreads, group_of, group_sum, group_best, Best, RedSlots (pn_group.h)

// the state: one allocation, see include/pathnet_hip.h
struct State {
    double *psum;       // [rows, C]
    double *hsum;       // [rows]
    int32_t *votes;     // [rows, C]
    int32_t *count;     // [rows]
    int32_t *bad;       // [rows]
};

__host__ __device__ inline State state_of(void *base, int64_t rows, int32_t C) {
    State st;
    char *p = (char *)base;
    st.psum = (double *)p;
    p += sizeof(double) * (size_t)rows * C;
    st.hsum = (double *)p;
    p += sizeof(double) * (size_t)rows;
    st.votes = (int32_t *)p;
    p += sizeof(int32_t) * (size_t)rows * C;
    st.count = (int32_t *)p;
    p += sizeof(int32_t) * (size_t)rows;
    st.bad = (int32_t *)p;
    return st;
}

__device__ inline double plogp(double p) { return p > 0.0 ? p * log(p) : 0.0; }

// ---- add ---------------------------------------------------------------------------------------------------------------------
// Scaled: e_c = exp((x_c - m) * inv) with inv = 1 / *tau; a *tau that is not finite and positive touches nothing and adds
// R * S (saturated) to status[0].  (x - m) * 1.0 is exact, so *tau == 1.0 leaves the bits of the plain kernel.
template <int G, bool Scaled>
__global__ __launch_bounds__(kThreads) void ensemble_add_kernel(const float *__restrict__ logits, int32_t R, int64_t S,
                                                                 int32_t C, const int32_t *__restrict__ index, int64_t rows,
                                                                 void *state, int32_t *status,
                                                                 const double *__restrict__ tau) {
    __shared__ RedSlots red;
    double inv = 1.0;
    if (Scaled) {
        const double t = *tau;
        if (!(t > 0.0 && t <= 1.7976931348623157e308)) {       // false for NaN, +inf, zero and negatives
            if (blockIdx.x == 0 && threadIdx.x == 0 && status) {
                const int64_t skipped = (int64_t)R * S;
                atomicAdd(status, (int32_t)(skipped < 2147483647LL ? skipped : 2147483647LL));
            }
            return;
        }
        inv = 1.0 / t;
    }
    const State st = state_of(state, rows, C);
    const int lane = G == 1 ? 0 : (int)(threadIdx.x % G);
    const int64_t per_block = kThreads / G;
    // (G = 256: s, and with it every `continue` below, is the same for the whole workgroup, so the barriers of its reductions
    //  stay paired; G = 64 reduces by shuffles alone, and s is uniform in a wave)
    for (int64_t s = (int64_t)blockIdx.x * per_block + threadIdx.x / G; s < S; s += (int64_t)gridDim.x * per_block) {
        int64_t row = s;
        if (index) {
            row = index[s];
            if (row < 0 || row >= rows) {
                if (lane == 0 && status) atomicAdd(status, R);     // R logits rows skipped
                continue;
            }
        }
        for (int32_t r = 0; r < R; r++) {
            const float *x = logits + ((int64_t)r * S + s) * C;
            Best<float> b{-INFINITY, C, 0};
            for (int32_t c = lane; c < C; c += G) {
                const float v = x[c];
                if (fabsf(v) <= 3.4028234663852886e38f) best_merge(b, v, c, 0);     // false for NaN and both infinities
                else b.flag = 1;
            }
            b = group_best<G>(b, red.bf);
            if (b.flag) {
                if (lane == 0) st.bad[row] += 1;
                continue;
            }
            const double m = (double)b.key;
            double z = 0.0;
            for (int32_t c = lane; c < C; c += G) z += exp(Scaled ? ((double)x[c] - m) * inv : (double)x[c] - m);
            z = group_sum<G>(z, red.d);
            double h = 0.0;
            for (int32_t c = lane; c < C; c += G) {
                const double p = exp(Scaled ? ((double)x[c] - m) * inv : (double)x[c] - m) / z;
                st.psum[row * C + c] += p;
                h += plogp(p);
            }
            h = group_sum<G>(h, red.d);
            if (lane == 0) {
                st.hsum[row] += -h;
                st.votes[row * C + b.c] += 1;
                st.count[row] += 1;
            }
        }
    }
}

// ---- finish ------------------------------------------------------------------------------------------------------------------
struct FinishParams {
    int64_t rows;           // rows of the state
    int64_t n;              // rows to finish: subset_rows with a subset, else rows
    int32_t C;
    const void *state;
    const int32_t *subset;
    const int64_t *target;
    pn_ensemble_out o;
};

template <int G>
__global__ __launch_bounds__(kThreads) void ensemble_finish_kernel(FinishParams fp) {
    __shared__ RedSlots red;
    const int32_t C = fp.C;
    const State st = state_of(const_cast<void *>(fp.state), fp.rows, C);
    const pn_ensemble_out &o = fp.o;
    const int lane = G == 1 ? 0 : (int)(threadIdx.x % G);
    const int64_t per_block = kThreads / G;
    for (int64_t j = (int64_t)blockIdx.x * per_block + threadIdx.x / G; j < fp.n; j += (int64_t)gridDim.x * per_block) {
        int64_t row = fp.subset ? (int64_t)fp.subset[j] : j;
        if (row < 0 || row >= fp.rows) row = -1;           // a subset entry outside the state: an empty row
        const int32_t cnt = row >= 0 ? st.count[row] : 0;
        const bool live = cnt > 0;
        Best<double> bp{-INFINITY, C, 0};
        Best<int32_t> bv{-1, C, 0};
        double h = 0.0;
        if (live)
            for (int32_t c = lane; c < C; c += G) {
                const double ps = st.psum[row * C + c];
                best_merge(bp, ps, c, 0);
                best_merge(bv, st.votes[row * C + c], c, 0);
                const double p = ps / (double)cnt;
                h += plogp(p);
                if (o.prob) o.prob[j * C + c] = (float)p;
            }
        else if (o.prob)
            for (int32_t c = lane; c < C; c += G) o.prob[j * C + c] = 0.0f;
        bp = group_best<G>(bp, red.bd);
        bv = group_best<G>(bv, red.bi);
        h = group_sum<G>(h, red.d);
        if (lane != 0) continue;
        // (bp.c == C: no class compared greater than -inf, which only a state that was written to from outside can hold)
        const int64_t label = live && bp.c < C ? bp.c : -1;
        if (o.label) o.label[j] = label;
        if (o.vote_label) o.vote_label[j] = live && bv.c < C ? bv.c : -1;
        const double ent = live ? -h : 0.0;
        if (o.confidence) o.confidence[j] = label >= 0 ? (float)(bp.key / (double)cnt) : 0.0f;
        if (o.entropy) o.entropy[j] = (float)ent;
        if (o.mutual_info) {
            const double mi = live ? ent - st.hsum[row] / (double)cnt : 0.0;
            o.mutual_info[j] = (float)(mi > 0.0 ? mi : 0.0);
        }
        if (o.agreement) o.agreement[j] = label >= 0 ? (float)((double)st.votes[row * C + label] / (double)cnt) : 0.0f;
        if (fp.target && (o.confusion || o.skipped)) {
            // (a subset entry outside the state has no target to read: it counts as label -1 alone)
            const int64_t t = row >= 0 ? fp.target[row] : 0;
            const bool t_ok = t >= 0 && t < C;
            if (row >= 0 && !t_ok) {
                if (o.skipped) atomicAdd((unsigned long long *)&o.skipped[0], 1ULL);
            }
            if (label < 0) {
                if (o.skipped) atomicAdd((unsigned long long *)&o.skipped[1], 1ULL);
            }
            if (row >= 0 && t_ok && label >= 0 && o.confusion)
                atomicAdd((unsigned long long *)&o.confusion[t * C + label], 1ULL);
        }
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
int check_shape(const char *who, int64_t rows, int32_t C) {
    if (C < 1 || C > kMaxC) PN_FAIL(PN_ERR_ARG, "%s: %d classes, 1 .. %d", who, C, kMaxC);
    if (rows < 0 || rows > 2147483647LL) PN_FAIL(PN_ERR_ARG, "%s: %lld rows, 0 .. 2^31 - 1", who, (long long)rows);
    return PN_OK;
}

template <bool Scaled>
int launch_add(const char *who, pn_context *ctx, const float *logits, int32_t R, int64_t S, int32_t C, const int32_t *index,
               int64_t rows, void *state, int32_t *status, const double *tau, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_shape(who, rows, C)) return rc;
    if (R < 1) PN_FAIL(PN_ERR_ARG, "%s: %d samples, at least 1", who, R);
    if (S < 0 || S > 2147483647LL) PN_FAIL(PN_ERR_ARG, "%s: %lld logits rows, 0 .. 2^31 - 1", who, (long long)S);
    if (!index && S > rows)
        PN_FAIL(PN_ERR_ARG, "%s: %lld logits rows for a state of %lld and no index", who, (long long)S, (long long)rows);
    if (S > 0 && rows > 0 && (!logits || !state)) PN_FAIL(PN_ERR_ARG, "%s: null logits or state", who);
    if (int rc = pn::context_check_device(ctx)) return rc;
    if (S == 0 || rows == 0) return PN_OK;
    const int G = group_of(C);
    const dim3 grid(blocks_for(S, G)), block(kThreads);
    if (G == 1)
        hipLaunchKernelGGL((ensemble_add_kernel<1, Scaled>), grid, block, 0, stream, logits, R, S, C, index, rows, state,
                           status, tau);
    else if (G == 64)
        hipLaunchKernelGGL((ensemble_add_kernel<64, Scaled>), grid, block, 0, stream, logits, R, S, C, index, rows, state,
                           status, tau);
    else
        hipLaunchKernelGGL((ensemble_add_kernel<256, Scaled>), grid, block, 0, stream, logits, R, S, C, index, rows, state,
                           status, tau);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

}  // namespace

extern "C" {

int pn_ensemble_state_bytes(int64_t rows, int32_t C, int64_t *bytes) {
    if (!bytes) PN_FAIL(PN_ERR_ARG, "pn_ensemble_state_bytes: null result");
    if (int rc = check_shape("pn_ensemble_state_bytes", rows, C)) return rc;
    *bytes = rows * (12 * (int64_t)C + 16);       // psum 8C + hsum 8 + votes 4C + count 4 + bad 4
    return PN_OK;
}

int pn_ensemble_route(int64_t rows, int32_t C, int32_t *route) {
    if (!route) PN_FAIL(PN_ERR_ARG, "pn_ensemble_route: null result");
    if (int rc = check_shape("pn_ensemble_route", rows, C)) return rc;
    const int G = group_of(C);
    *route = rows == 0 ? PN_ENSEMBLE_ROUTE_NONE
                       : G == 1 ? PN_ENSEMBLE_ROUTE_THREAD : G == 64 ? PN_ENSEMBLE_ROUTE_WAVE : PN_ENSEMBLE_ROUTE_BLOCK;
    return PN_OK;
}

int pn_ensemble_add(pn_context *ctx, const float *logits, int32_t R, int64_t S, int32_t C, const int32_t *index, int64_t rows,
                    void *state, int32_t *status, void *stream_) {
    return launch_add<false>("pn_ensemble_add", ctx, logits, R, S, C, index, rows, state, status, nullptr, stream_);
}

int pn_ensemble_add_scaled(pn_context *ctx, const float *logits, int32_t R, int64_t S, int32_t C, const int32_t *index,
                           int64_t rows, void *state, int32_t *status, const double *tau, void *stream_) {
    if (!tau) PN_FAIL(PN_ERR_ARG, "pn_ensemble_add_scaled: null tau");
    return launch_add<true>("pn_ensemble_add_scaled", ctx, logits, R, S, C, index, rows, state, status, tau, stream_);
}

int pn_ensemble_finish(pn_context *ctx, int64_t rows, int32_t C, const void *state, const int32_t *subset, int64_t subset_rows,
                       const int64_t *target, const pn_ensemble_out *out, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_shape("pn_ensemble_finish", rows, C)) return rc;
    if (!out) PN_FAIL(PN_ERR_ARG, "pn_ensemble_finish: null output description");
    if (subset_rows < 0 || subset_rows > 2147483647LL || (!subset && subset_rows != 0))
        PN_FAIL(PN_ERR_ARG, "pn_ensemble_finish: %lld subset rows%s", (long long)subset_rows, subset ? "" : " without a subset");
    if (!target && (out->confusion || out->skipped))
        PN_FAIL(PN_ERR_ARG, "pn_ensemble_finish: confusion / skipped asked for without a target");
    const int64_t n = subset ? subset_rows : rows;
    if (n > 0 && rows > 0 && !state) PN_FAIL(PN_ERR_ARG, "pn_ensemble_finish: null state");
    if (int rc = pn::context_check_device(ctx)) return rc;
    if (n == 0) return PN_OK;
    FinishParams fp{};
    fp.rows = rows;
    fp.n = n;
    fp.C = C;
    fp.state = state;
    fp.subset = subset;
    fp.target = target;
    fp.o = *out;
    const int G = group_of(C);
    const dim3 grid(blocks_for(n, G)), block(kThreads);
    if (G == 1)
        hipLaunchKernelGGL(ensemble_finish_kernel<1>, grid, block, 0, stream, fp);
    else if (G == 64)
        hipLaunchKernelGGL(ensemble_finish_kernel<64>, grid, block, 0, stream, fp);
    else
        hipLaunchKernelGGL(ensemble_finish_kernel<256>, grid, block, 0, stream, fp);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

}  // extern "C"
