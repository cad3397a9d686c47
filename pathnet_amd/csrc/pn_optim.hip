// pn_optim.hip -- the optimizer's options on the tail of the training step (include/pathnet_hip.h, "optimizer options"):
// the global gradient norm, Adam / AdamW / amsgrad with the clip fused into the read of the gradient, a learning-rate
// schedule evaluated on the device, a non-finite guard, and the stand-alone in-place clip.  pn_adam_step (pn_train.hip) is
// the option-less update and is not touched.  gfx950 only.
//
// How the norm travels: grad_sumsq_kernel's workgroups each store ONE double into the state buffer; the launches behind
// it (adam_ex_kernel, grad_scale_kernel) begin by summing those partials, every workgroup for itself in one fixed order.  The
// kernel boundary between the two makes the partials visible, every workgroup gets the same bits, and no workgroup of
// this file waits for, spins on or counts against another (the one ticket is pn_adam_step_advance's, unchanged).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/pathnet_hip.h"
#include "pn_internal.h"
#include "pn_step_state.h"

namespace {

constexpr int OPT_CHUNK = 2048;         // elements per chunk (= a workgroup's share in the update, as in adam_kernel)
constexpr int OPT_THREADS = 256;
constexpr int OPT_GRID_CAP = 256;       // workgroups per grad_sumsq launch = partial sums per launch, at most

inline double *partials_of(void *state) { return reinterpret_cast<double *>(static_cast<pn_optim_report *>(state) + 1); }

// ---- sum of squares of a list of gradients -------------------------------------------------------------------------
struct GradList {
    float *grad[PN_ADAM_MAX_TENSORS];
    long long count[PN_ADAM_MAX_TENSORS];
    int chunk_begin[PN_ADAM_MAX_TENSORS + 1];
    int n;
    pn_optim_report *rep;
    double *partial;        // this launch's range of the state's partials (sumsq) / all of them (scale)
    int n_partials;         // sumsq: the total of the call, stored into rep by the first launch (-1: not this launch)
    float max_norm;         // scale
};

// the sum of one double per thread over the workgroup, in one fixed order: the lanes of a wavefront (xor butterfly), then
// the four wavefronts in order, read back by every thread -- the same bits in every thread.  `part` is used once per kernel.
__device__ __forceinline__ double block_sum(double mine, double *part) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < OPT_THREADS / 64; w++) s += part[w];
    return s;
}

// thread i of chunk c takes elements i, i + 256, ...; the chunks of a workgroup in order; then block_sum: one fixed order
// for a given list, whatever the run
__global__ __launch_bounds__(OPT_THREADS) void grad_sumsq_kernel(GradList a) {
    __shared__ double part[OPT_THREADS / 64];
    const int chunks = a.chunk_begin[a.n];
    double mine = 0.0;
    int k = 0;
    for (int c = blockIdx.x; c < chunks; c += gridDim.x) {      // (block-uniform)
        while (k + 1 < a.n && c >= a.chunk_begin[k + 1]) k++;
        const float *g = a.grad[k];
        const long long count = a.count[k];
        const long long base = (long long)(c - a.chunk_begin[k]) * OPT_CHUNK;
        for (int i = threadIdx.x; i < OPT_CHUNK; i += OPT_THREADS) {
            const long long e = base + i;
            if (e >= count) break;
            const double x = (double)g[e];
            mine += x * x;
        }
    }
    const double s = block_sum(mine, part);
    if (threadIdx.x == 0) {
        a.partial[blockIdx.x] = s;
        if (blockIdx.x == 0 && a.n_partials >= 0) a.rep->n_partials = a.n_partials;
    }
}

// the partials of the launch(es) before this one: thread i takes partials i, i + 256, ... in order (one each, for lists of
// up to 32 tensors), then block_sum.  Every workgroup does exactly this, so every workgroup holds the same bits.  (One
// thread adding them in index order costs ~10 us at 200 partials, on every workgroup's critical path: measured, and dropped.)
__device__ __forceinline__ double sum_partials(const pn_optim_report *rep, double *part) {
    const double *partial = reinterpret_cast<const double *>(rep + 1);
    const int n = rep->n_partials;
    double mine = 0.0;
    for (int i = threadIdx.x; i < n; i += OPT_THREADS) mine += partial[i];
    return block_sum(mine, part);
}

// clip_grad_norm_'s coefficient, formed in double and converted once.  max_norm = +inf gives exactly 1.
__device__ __forceinline__ float clip_coef(double norm, float max_norm) {
    return (float)fmin(1.0, (double)max_norm / (norm + 1e-6));
}

// ---- grad *= coef: the stand-alone clip ---------------------------------------------------------------------------
__global__ __launch_bounds__(OPT_THREADS) void grad_scale_kernel(GradList a, int report) {
    __shared__ double part[OPT_THREADS / 64];
    const double sumsq = sum_partials(a.rep, part);
    const bool finite = isfinite(sumsq);
    const double norm = sqrt(sumsq);
    const float coef = finite ? clip_coef(norm, a.max_norm) : 1.0f;
    if (report && blockIdx.x == 0 && threadIdx.x == 0) {
        a.rep->grad_norm = norm;
        a.rep->clip_coef = coef;
    }
    if (!finite || coef == 1.0f || a.n == 0) return;        // (block-uniform) nothing to scale
    int k = 0;
    while (k + 1 < a.n && (int)blockIdx.x >= a.chunk_begin[k + 1]) k++;
    float *g = a.grad[k];
    const long long count = a.count[k];
    const long long base = (long long)((int)blockIdx.x - a.chunk_begin[k]) * OPT_CHUNK;
    for (int i = threadIdx.x; i < OPT_CHUNK; i += OPT_THREADS) {
        const long long e = base + i;
        if (e >= count) break;
        g[e] *= coef;
    }
}

// ---- the option-aware update ---------------------------------------------------------------------------------------
struct AdamExList {
    pn_adam_tensor_ex t[PN_ADAM_MAX_TENSORS];
    int block_begin[PN_ADAM_MAX_TENSORS + 1];
    int n;
    float lr, beta1, beta2, eps, weight_decay;
    pn_optim_spec spec;
    pn_optim_report *rep;           // or null
    long long step;                 // without dyn
    const pn_step_state *dyn;       // the step count in device memory
    int advance;                    // the step's last launch: the workgroup that finishes last moves *dyn on
    int report;                     // the step's first launch: workgroup 0 writes the report
};

// b^n by squaring (n < 2^31): the bias corrections, as adam_kernel forms them
__device__ __forceinline__ void pow2_by_squaring(double b1, double b2, long long n, double &p1, double &p2) {
    p1 = p2 = 1.0;
    while (n > 0) {
        if (n & 1) {
            p1 *= b1;
            p2 *= b2;
        }
        b1 *= b1;
        b2 *= b2;
        n >>= 1;
    }
}

// lr * warm(e) * decay(max(e - warmup_steps, 0)) in double (the header has the formulas)
__device__ __forceinline__ double scheduled_lr(const pn_optim_spec &o, double lr, long long step) {
    const long long e = step > 1 ? step - 1 : 0;
    double warm = 1.0;
    if (o.warmup_steps > 0) {
        const long long w = e < o.warmup_steps ? e : o.warmup_steps;
        warm = o.start_factor + (1.0 - o.start_factor) * (double)w / (double)o.warmup_steps;
    }
    const long long d = e > o.warmup_steps ? e - o.warmup_steps : 0;
    double decay = 1.0;
    if (o.schedule == PN_LR_STEP)
        decay = pow(o.gamma, (double)(d / o.step_size));
    else if (o.schedule == PN_LR_EXPONENTIAL)
        decay = pow(o.gamma, (double)d);
    else if (o.schedule == PN_LR_COSINE && lr > 0.0) {
        const long long c = d < o.t_max ? d : o.t_max;
        decay = (o.lr_min + (lr - o.lr_min) * (1.0 + cospi((double)c / (double)o.t_max)) / 2.0) / lr;
    }
    return lr * warm * decay;
}

__global__ __launch_bounds__(OPT_THREADS) void adam_ex_kernel(AdamExList a) {
    __shared__ double part[OPT_THREADS / 64];
    // ---- block-uniform: the step's scalars, in double, converted once
    const long long step = a.dyn ? (long long)a.dyn->adam_step : a.step;
    const bool clip = a.spec.max_grad_norm != 0.0f;
    double norm = NAN;
    float coef = 1.0f;
    bool skip = false;
    if (clip) {
        const double sumsq = sum_partials(a.rep, part);
        norm = sqrt(sumsq);
        skip = !isfinite(sumsq);
        if (!skip) coef = clip_coef(norm, a.spec.max_grad_norm);
    }
    const double lr_now = scheduled_lr(a.spec, (double)a.lr, step);
    double p1, p2;
    pow2_by_squaring((double)a.beta1, (double)a.beta2, step, p1, p2);
    const float lr_over_bc1 = (float)(lr_now / (1.0 - p1));
    const float inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - p2));
    const bool decoupled = (a.spec.flags & PN_OPTIM_DECOUPLED_WD) != 0, amsgrad = (a.spec.flags & PN_OPTIM_AMSGRAD) != 0;
    const float keep = decoupled ? (float)(1.0 - lr_now * (double)a.weight_decay) : 1.0f;
    const float l2 = decoupled ? 0.0f : a.weight_decay;
    if (a.report && a.rep && blockIdx.x == 0 && threadIdx.x == 0) {
        a.rep->grad_norm = norm;
        a.rep->lr = lr_now;
        a.rep->clip_coef = coef;
        if (skip) a.rep->skipped += 1;
    }
    if (!skip && a.n > 0) {
        int k = 0;
        while (k + 1 < a.n && (int)blockIdx.x >= a.block_begin[k + 1]) k++;
        const pn_adam_tensor_ex t = a.t[k];
        const long long base = (long long)((int)blockIdx.x - a.block_begin[k]) * OPT_CHUNK;
        for (int i = threadIdx.x; i < OPT_CHUNK; i += OPT_THREADS) {
            const long long e = base + i;
            if (e >= t.count) break;
            float g = coef * t.grad[e];
            float p = t.param[e];
            if (decoupled)
                p *= keep;
            else
                g += l2 * p;
            const float m = a.beta1 * t.exp_avg[e] + (1.0f - a.beta1) * g;
            const float v = a.beta2 * t.exp_avg_sq[e] + (1.0f - a.beta2) * g * g;
            t.exp_avg[e] = m;
            t.exp_avg_sq[e] = v;
            float vd = v;
            if (amsgrad) {
                vd = fmaxf(t.max_exp_avg_sq[e], v);
                t.max_exp_avg_sq[e] = vd;
            }
            t.param[e] = p - lr_over_bc1 * (m / (sqrtf(vd) * inv_sqrt_bc2 + a.eps));
        }
    }
    if (a.dyn && a.advance) {       // pn_adam_step_advance's ticket: every workgroup has read adam_step by the time it takes one
        __syncthreads();
        if (threadIdx.x == 0) {
            pn_step_state *s = const_cast<pn_step_state *>(a.dyn);
            unsigned int *ticket = reinterpret_cast<unsigned int *>(&s->reserved);
            if (atomicAdd(ticket, 1u) == gridDim.x - 1) {
                atomicExch(ticket, 0u);
                pn::advance_step_state(s);
            }
        }
    }
}

int check_spec(const pn_optim_spec *o, float lr, const char *who) {
    if (!o) PN_FAIL(PN_ERR_ARG, "%s: null spec", who);
    if (o->flags & ~(PN_OPTIM_DECOUPLED_WD | PN_OPTIM_AMSGRAD | PN_OPTIM_NO_REPORT))
        PN_FAIL(PN_ERR_ARG, "%s: unknown flags 0x%x", who, (unsigned)o->flags);
    if (!(o->max_grad_norm >= 0.0f)) PN_FAIL(PN_ERR_ARG, "%s: max_grad_norm %g", who, (double)o->max_grad_norm);
    if (o->warmup_steps < 0 || !(o->start_factor >= 0.0 && o->start_factor <= 1.0))
        PN_FAIL(PN_ERR_ARG, "%s: warmup_steps %lld, start_factor %g", who, (long long)o->warmup_steps, o->start_factor);
    switch (o->schedule) {
    case PN_LR_CONSTANT:
        break;
    case PN_LR_STEP:
        if (o->step_size < 1) PN_FAIL(PN_ERR_ARG, "%s: step_size %lld", who, (long long)o->step_size);
        [[fallthrough]];
    case PN_LR_EXPONENTIAL:
        if (!(o->gamma > 0.0) || !std::isfinite(o->gamma)) PN_FAIL(PN_ERR_ARG, "%s: gamma %g", who, o->gamma);
        break;
    case PN_LR_COSINE:
        if (o->t_max < 1) PN_FAIL(PN_ERR_ARG, "%s: t_max %lld", who, (long long)o->t_max);
        if (!(o->lr_min >= 0.0 && o->lr_min <= (double)lr)) PN_FAIL(PN_ERR_ARG, "%s: lr_min %g outside [0, lr = %g]", who, o->lr_min, (double)lr);
        break;
    default:
        PN_FAIL(PN_ERR_ARG, "%s: schedule %d is no PN_LR_* value", who, (int)o->schedule);
    }
    return PN_OK;
}

int check_list(const pn_adam_tensor *tensors, int32_t n_tensors, const void *state, const char *who) {
    if (n_tensors < 0 || (n_tensors > 0 && !tensors)) PN_FAIL(PN_ERR_ARG, "%s: bad tensor list", who);
    if (!state) PN_FAIL(PN_ERR_ARG, "%s: null state buffer", who);
    for (int32_t i = 0; i < n_tensors; i++)
        if (tensors[i].count < 0 || (tensors[i].count > 0 && !tensors[i].grad))
            PN_FAIL(PN_ERR_ARG, "%s: tensor %d has a null gradient", who, i);
    return PN_OK;
}

// tensors [at, at + a.n) as a chunk table -> the chunk count
int fill_grad_list(GradList &a, const pn_adam_tensor *tensors, int32_t n_tensors, int32_t at) {
    a.n = n_tensors - at < PN_ADAM_MAX_TENSORS ? n_tensors - at : PN_ADAM_MAX_TENSORS;
    int chunks = 0;
    for (int i = 0; i < a.n; i++) {
        a.grad[i] = const_cast<float *>(tensors[at + i].grad);
        a.count[i] = tensors[at + i].count;
        a.chunk_begin[i] = chunks;
        chunks += (int)((tensors[at + i].count + OPT_CHUNK - 1) / OPT_CHUNK);
    }
    a.chunk_begin[a.n] = chunks;
    return chunks;
}

// one launch per PN_ADAM_MAX_TENSORS tensors, each writing the partials behind those of the launch before it; a list
// without an element still gets its one partial (0)
int launch_grad_sumsq(const pn_adam_tensor *tensors, int32_t n_tensors, void *state, hipStream_t stream) {
    pn_optim_report *rep = static_cast<pn_optim_report *>(state);
    int total = 0;
    for (int32_t at = 0; at < n_tensors; at += PN_ADAM_MAX_TENSORS) {
        GradList a{};
        const int chunks = fill_grad_list(a, tensors, n_tensors, at);
        total += chunks < OPT_GRID_CAP ? chunks : OPT_GRID_CAP;
    }
    if (total == 0) {       // no element anywhere: one workgroup over an empty list stores the one partial
        GradList a{};
        a.rep = rep;
        a.partial = partials_of(state);
        a.n_partials = 1;
        hipLaunchKernelGGL(grad_sumsq_kernel, dim3(1), dim3(OPT_THREADS), 0, stream, a);
        PN_CHECK_HIP(hipGetLastError());
        return PN_OK;
    }
    int done = 0;
    for (int32_t at = 0; at < n_tensors; at += PN_ADAM_MAX_TENSORS) {
        GradList a{};
        const int chunks = fill_grad_list(a, tensors, n_tensors, at);
        const int blocks = chunks < OPT_GRID_CAP ? chunks : OPT_GRID_CAP;
        if (blocks == 0) continue;
        a.rep = rep;
        a.partial = partials_of(state) + done;
        a.n_partials = done == 0 ? total : -1;
        hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks), dim3(OPT_THREADS), 0, stream, a);
        PN_CHECK_HIP(hipGetLastError());
        done += blocks;
    }
    return PN_OK;
}

int adam_ex_impl(const pn_adam_tensor_ex *tensors, int32_t n_tensors, float lr, float beta1, float beta2, float eps,
                 float weight_decay, const pn_optim_spec *spec, void *state, int64_t step, const pn_step_state *step_state,
                 bool advance, void *stream_) {
    const char *who = advance ? "pn_adam_step_ex_advance" : "pn_adam_step_ex";
    if (n_tensors < 0 || (n_tensors > 0 && !tensors)) PN_FAIL(PN_ERR_ARG, "%s: bad tensor list", who);
    if (int rc = check_spec(spec, lr, who)) return rc;
    if (spec->max_grad_norm != 0.0f && !state) PN_FAIL(PN_ERR_ARG, "%s: max_grad_norm needs the state buffer", who);
    if (advance && !step_state) PN_FAIL(PN_ERR_ARG, "%s: no step state to advance", who);
    if (step_state) step = 1;       // (ignored: the kernel reads step_state->adam_step)
    if (step < 1) PN_FAIL(PN_ERR_ARG, "%s: step counts from 1 (got %lld)", who, (long long)step);
    const bool amsgrad = (spec->flags & PN_OPTIM_AMSGRAD) != 0;
    for (int32_t i = 0; i < n_tensors; i++) {
        const pn_adam_tensor_ex &t = tensors[i];
        if (t.count < 0 || (t.count > 0 && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq || (amsgrad && !t.max_exp_avg_sq))))
            PN_FAIL(PN_ERR_ARG, "%s: tensor %d has a null pointer", who, i);
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    bool report = state && !(spec->flags & PN_OPTIM_NO_REPORT);
    const int32_t launches = n_tensors > 0 ? (n_tensors + PN_ADAM_MAX_TENSORS - 1) / PN_ADAM_MAX_TENSORS : 1;
    for (int32_t l = 0; l < launches; l++) {
        const int32_t at = l * PN_ADAM_MAX_TENSORS;
        const bool last = l == launches - 1;
        AdamExList a{};
        a.n = n_tensors - at < PN_ADAM_MAX_TENSORS ? n_tensors - at : PN_ADAM_MAX_TENSORS;
        int blocks = 0;
        for (int i = 0; i < a.n; i++) {
            a.t[i] = tensors[at + i];
            a.block_begin[i] = blocks;
            blocks += (int)((tensors[at + i].count + OPT_CHUNK - 1) / OPT_CHUNK);
        }
        a.block_begin[a.n] = blocks;
        if (blocks == 0) {
            // a launch without elements runs only for what else the step's last launch must carry: a report that no launch
            // has written yet, the advance
            if (!(last && (report || advance))) continue;
            a.n = 0;
            blocks = 1;
        }
        a.lr = lr;
        a.beta1 = beta1;
        a.beta2 = beta2;
        a.eps = eps;
        a.weight_decay = weight_decay;
        a.spec = *spec;
        a.rep = static_cast<pn_optim_report *>(state);
        a.step = step;
        a.dyn = step_state;
        a.advance = (advance && last) ? 1 : 0;
        a.report = report ? 1 : 0;
        hipLaunchKernelGGL(adam_ex_kernel, dim3(blocks), dim3(OPT_THREADS), 0, stream, a);
        PN_CHECK_HIP(hipGetLastError());
        report = false;
    }
    return PN_OK;
}

}  // namespace

extern "C" {

int pn_optim_state_bytes(int64_t total_elements, int32_t n_tensors, int64_t *bytes) {
    if (!bytes || total_elements < 0 || n_tensors < 0)
        PN_FAIL(PN_ERR_ARG, "pn_optim_state_bytes: total_elements=%lld n_tensors=%d", (long long)total_elements, n_tensors);
    const int64_t launches = n_tensors > 0 ? (n_tensors + PN_ADAM_MAX_TENSORS - 1) / PN_ADAM_MAX_TENSORS : 1;
    *bytes = (int64_t)sizeof(pn_optim_report) + launches * OPT_GRID_CAP * (int64_t)sizeof(double);
    return PN_OK;
}

int pn_grad_norm(const pn_adam_tensor *tensors, int32_t n_tensors, void *state, void *stream) {
    if (int rc = check_list(tensors, n_tensors, state, "pn_grad_norm")) return rc;
    return launch_grad_sumsq(tensors, n_tensors, state, static_cast<hipStream_t>(stream));
}

int pn_adam_step_ex(const pn_adam_tensor_ex *tensors, int32_t n_tensors, float lr, float beta1, float beta2, float eps,
                    float weight_decay, const pn_optim_spec *spec, void *state, int64_t step, const pn_step_state *step_state,
                    void *stream) {
    return adam_ex_impl(tensors, n_tensors, lr, beta1, beta2, eps, weight_decay, spec, state, step, step_state, false, stream);
}

int pn_adam_step_ex_advance(const pn_adam_tensor_ex *tensors, int32_t n_tensors, float lr, float beta1, float beta2,
                            float eps, float weight_decay, const pn_optim_spec *spec, void *state,
                            pn_step_state *step_state, void *stream) {
    return adam_ex_impl(tensors, n_tensors, lr, beta1, beta2, eps, weight_decay, spec, state, 1, step_state, true, stream);
}

int pn_clip_grad_norm(const pn_adam_tensor *tensors, int32_t n_tensors, float max_norm, void *state, void *stream_) {
    if (int rc = check_list(tensors, n_tensors, state, "pn_clip_grad_norm")) return rc;
    if (!(max_norm > 0.0f)) PN_FAIL(PN_ERR_ARG, "pn_clip_grad_norm: max_norm %g", (double)max_norm);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int rc = launch_grad_sumsq(tensors, n_tensors, state, stream)) return rc;
    bool report = true;
    const int32_t launches = n_tensors > 0 ? (n_tensors + PN_ADAM_MAX_TENSORS - 1) / PN_ADAM_MAX_TENSORS : 1;
    for (int32_t l = 0; l < launches; l++) {
        const int32_t at = l * PN_ADAM_MAX_TENSORS;
        GradList a{};
        int blocks = fill_grad_list(a, tensors, n_tensors, at);
        if (blocks == 0) {
            if (!(l == launches - 1 && report)) continue;
            a.n = 0;                // nothing to scale anywhere: the launch only writes the report
            blocks = 1;
        }
        a.rep = static_cast<pn_optim_report *>(state);
        a.partial = partials_of(state);
        a.max_norm = max_norm;
        hipLaunchKernelGGL(grad_scale_kernel, dim3(blocks), dim3(OPT_THREADS), 0, stream, a, report ? 1 : 0);
        PN_CHECK_HIP(hipGetLastError());
        report = false;
    }
    return PN_OK;
}

}  // extern "C"
