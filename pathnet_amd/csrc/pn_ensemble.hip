// pn_ensemble.hip -- ensemble prediction over resampled paths (pn_ensemble_add / pn_ensemble_finish).
//
// A PathNet prediction depends on the W paths the sampler drew for the node.  K independent draws give K logit rows per
// node; this file averages their class probabilities where they are and says how much the draws disagree.
//
//   ensemble_add_kernel<G>     logits [R, S, C] fp32 -> the caller's state (psum, hsum, votes, count, bad).  ONE group of G
//                              threads owns state row index[s] and takes its R samples in ascending r, so no floating-point
//                              atomic exists and one [R, S, C] call leaves the bits of R calls of [1, S, C].
//   ensemble_finish_kernel<G>  state -> prob, label, vote_label, confidence, entropy, mutual_info, agreement, and with a
//                              target the confusion matrix (integer atomics: exact, order-free).
//
// Work split (pn_ensemble_route): G depends on C alone.
//   C <= 16           G = 1    a thread per row: the class loop is the ascending serial sum
//   16 < C <= 1024    G = 64   a wave per row, four rows per workgroup: lane l holds classes l, l + 64, ...
//   1024 < C <= 4096  G = 256  a workgroup per row
// Order of a sum over classes: every lane adds its own classes in ascending c, the 64 lane sums meet in a butterfly
// (xor 32, 16, ..., 1: fp addition commutes, so every lane holds the same bits), the four wave sums of a workgroup are added
// as (w0 + w1) + (w2 + w3).  That order is a function of C and nothing else -- not of S, R, rows, the grid or the index --
// and for G = 1 it is the plain ascending sum.  All arithmetic after the fp32 -> fp64 conversion of a logit is fp64.
// Plain C++ and vector stores only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pn_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1 << 16;          // rows beyond that are taken in a grid-stride loop
constexpr int kThreadMaxC = 16;              // C <= 16: a thread per row
constexpr int kWaveMaxC = 1024;              // C <= 1024: a wave per row
constexpr int kMaxC = 4096;

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

// ---- reductions over the G threads that own a row; every thread returns the same bits -------------------------------------
// G = 256 goes through LDS: `red` holds one slot per wave, and every thread of the workgroup must make the call.
template <int G>
__device__ inline double group_sum(double v, double *red) {
    if (G == 1) return v;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if (G == 256) {
        __syncthreads();        // (the previous reduction's readers are done with `red`)
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        v = (red[0] + red[1]) + (red[2] + red[3]);
    }
    return v;
}

// the largest key and the lowest class that holds it, with a flag OR-ed alongside
template <typename T>
struct Best {
    T key;
    int32_t c;
    int32_t flag;
};

template <typename T>
__device__ inline void best_merge(Best<T> &a, T key, int32_t c, int32_t flag) {
    if (key > a.key || (key == a.key && c < a.c)) {
        a.key = key;
        a.c = c;
    }
    a.flag |= flag;
}

template <int G, typename T>
__device__ inline Best<T> group_best(Best<T> b, Best<T> *red) {
    if (G == 1) return b;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const T key = __shfl_xor(b.key, m, 64);
        const int32_t c = __shfl_xor(b.c, m, 64);
        const int32_t flag = __shfl_xor(b.flag, m, 64);
        best_merge(b, key, c, flag);
    }
    if (G == 256) {
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = b;
        __syncthreads();
        b = red[0];
#pragma unroll
        for (int w = 1; w < 4; w++) best_merge(b, red[w].key, red[w].c, red[w].flag);
    }
    return b;
}

union RedSlots {            // the LDS of one workgroup: four slots, reused by every reduction
    double d[4];
    Best<float> bf[4];
    Best<double> bd[4];
    Best<int32_t> bi[4];
};

__device__ inline double plogp(double p) { return p > 0.0 ? p * log(p) : 0.0; }

// ---- add ---------------------------------------------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(kThreads) void ensemble_add_kernel(const float *__restrict__ logits, int32_t R, int64_t S,
                                                                 int32_t C, const int32_t *__restrict__ index, int64_t rows,
                                                                 void *state, int32_t *status) {
    __shared__ RedSlots red;
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
            for (int32_t c = lane; c < C; c += G) z += exp((double)x[c] - m);
            z = group_sum<G>(z, red.d);
            double h = 0.0;
            for (int32_t c = lane; c < C; c += G) {
                const double p = exp((double)x[c] - m) / z;
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
int group_of(int32_t C) { return C <= kThreadMaxC ? 1 : C <= kWaveMaxC ? 64 : 256; }

int check_shape(const char *who, int64_t rows, int32_t C) {
    if (C < 1 || C > kMaxC) PN_FAIL(PN_ERR_ARG, "%s: %d classes, 1 .. %d", who, C, kMaxC);
    if (rows < 0 || rows > 2147483647LL) PN_FAIL(PN_ERR_ARG, "%s: %lld rows, 0 .. 2^31 - 1", who, (long long)rows);
    return PN_OK;
}

unsigned blocks_for(int64_t n, int G) {
    const int64_t per_block = kThreads / G;
    const int64_t need = (n + per_block - 1) / per_block;
    return (unsigned)(need < kMaxBlocks ? need : kMaxBlocks);
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
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_shape("pn_ensemble_add", rows, C)) return rc;
    if (R < 1) PN_FAIL(PN_ERR_ARG, "pn_ensemble_add: %d samples, at least 1", R);
    if (S < 0 || S > 2147483647LL) PN_FAIL(PN_ERR_ARG, "pn_ensemble_add: %lld logits rows, 0 .. 2^31 - 1", (long long)S);
    if (!index && S > rows)
        PN_FAIL(PN_ERR_ARG, "pn_ensemble_add: %lld logits rows for a state of %lld and no index", (long long)S, (long long)rows);
    if (S > 0 && rows > 0 && (!logits || !state)) PN_FAIL(PN_ERR_ARG, "pn_ensemble_add: null logits or state");
    if (int rc = pn::context_check_device(ctx)) return rc;
    if (S == 0 || rows == 0) return PN_OK;
    const int G = group_of(C);
    const dim3 grid(blocks_for(S, G)), block(kThreads);
    if (G == 1)
        hipLaunchKernelGGL(ensemble_add_kernel<1>, grid, block, 0, stream, logits, R, S, C, index, rows, state, status);
    else if (G == 64)
        hipLaunchKernelGGL(ensemble_add_kernel<64>, grid, block, 0, stream, logits, R, S, C, index, rows, state, status);
    else
        hipLaunchKernelGGL(ensemble_add_kernel<256>, grid, block, 0, stream, logits, R, S, C, index, rows, state, status);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
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
