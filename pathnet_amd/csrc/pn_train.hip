// pn_train.hip -- the two element-wise pieces of the reference's training step that sit between the aggregator's
// forward and backward: the loss and the optimizer update.
//   loss      torch.nn.CrossEntropyLoss()      /root/reference/PathNet_run.py:297, :346
//   update    torch.optim.Adam(lr, weight_decay)  PathNet_run.py:295-296, :352
// On the bench workload torch spends ~100 us per step on them (a single-block nll reduction, softmax forward and
// backward launches, a multi_tensor_apply Adam); both are one small launch here.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/pathnet_hip.h"
#include "pn_internal.h"
#include "pn_step_state.h"
#include "pn_loss.h"

namespace {

// ---- softmax cross entropy, mean over rows, and d loss / d logits -----------------------------------------------
// one wavefront per 64 rows is plenty for C <= a few hundred classes: a thread walks its row three times
__global__ __launch_bounds__(1024) void cross_entropy_kernel(const float *__restrict__ logits,
                                                             const int64_t *__restrict__ target, int rows, int classes,
                                                             float inv_rows, float *__restrict__ loss,
                                                             float *__restrict__ g_logits, int store) {
    __shared__ float part[16];
    float mine = 0.0f;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += gridDim.x * blockDim.x) {
        const float *x = logits + (int64_t)r * classes;
        float m = x[0];
        for (int c = 1; c < classes; c++) m = fmaxf(m, x[c]);
        float s = 0.0f;
        for (int c = 0; c < classes; c++) s += expf(x[c] - m);
        // log softmax as (x - m) - log(s): both terms are small whatever the size of the logits.  m + log(s) would be rounded
        // at the magnitude of the largest logit and every probability would carry ulp(max |x|) / 2 of relative error.
        const float ls = logf(s);
        // A target outside [0, classes) poisons the loss (NaN) and leaves a zero gradient row; no address is formed from
        // it: a clamped index and selects, no branch around a load (pool_step2_kernel, pn_pool_step2.inc, has the same lines)
        const int64_t t64 = target[r];
        const bool ok = t64 >= 0 && t64 < (int64_t)classes;
        const int t = ok ? (int)t64 : 0;
        const float row = ls - (x[t] - m);
        mine += ok ? row : NAN;
        if (g_logits) {
            float *g = g_logits + (int64_t)r * classes;
            for (int c = 0; c < classes; c++) {
                const float gv = (expf((x[c] - m) - ls) - (c == t ? 1.0f : 0.0f)) * inv_rows;
                g[c] = ok ? gv : 0.0f;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.0f;
        for (int w = 0; w < (int)(blockDim.x >> 6); w++) s += part[w];
        if (store)
            *loss = s * inv_rows;           // one workgroup computes the whole loss: no zero-fill launch ahead of it
        else
            atomicAdd(loss, s * inv_rows);  // (several workgroups, or a loss that accumulates over micro-batches)
    }
}

// ---- the same with pn_loss_spec's options (class weights, ignore_index, label smoothing; pn_loss.h has the row) ----------
// k = grad_scale / D or grad_scale is formed here from D in device memory: the launch carries no number that depends on
// the targets.  Same launch shape, same summation order as cross_entropy_kernel.
__global__ __launch_bounds__(1024) void cross_entropy_opts_kernel(const float *__restrict__ logits,
                                                                  const int64_t *__restrict__ target, int rows, int classes,
                                                                  pn::LossOpts o, float *__restrict__ loss,
                                                                  float *__restrict__ g_logits, int store) {
    __shared__ float part[16];
    float k_grad, k_loss;
    pn::loss_factors(o, k_grad, k_loss);
    float mine = 0.0f;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += gridDim.x * blockDim.x)
        mine += pn::ce_row_opts(logits + (int64_t)r * classes, classes, target[r], o, k_grad,
                                g_logits ? g_logits + (int64_t)r * classes : nullptr);
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) mine += __shfl_xor(mine, o2, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.0f;
        for (int w = 0; w < (int)(blockDim.x >> 6); w++) s += part[w];
        if (store)
            *loss = s * k_loss;
        else
            atomicAdd(loss, s * k_loss);
    }
}

// ---- D = sum over the kept rows of w[target]: one workgroup, thread i takes rows i, i + 1024, ... in order, then the
// wavefronts' and the sixteen partial sums in a fixed order -- the same bits in every run at any row count.  A row is kept
// when its target is a class and not the ignore value; the weight is read at a clamped index.
__global__ __launch_bounds__(1024) void loss_denominator_kernel(const int64_t *__restrict__ target, int rows, int classes,
                                                                pn::LossOpts o, float *__restrict__ denom) {
    __shared__ float part[16];
    float mine = 0.0f;
#pragma unroll 4
    for (int64_t r = threadIdx.x; r < rows; r += 1024) {
        const int64_t t64 = target[r];
        const bool kept = t64 >= 0 && t64 < (int64_t)classes && !(o.has_ignore && t64 == o.ignore);
        const int t = kept ? (int)t64 : 0;
        const float w = o.weight ? o.weight[t] : 1.0f;
        mine += kept ? w : 0.0f;
    }
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) mine += __shfl_xor(mine, o2, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.0f;
        for (int w = 0; w < 16; w++) s += part[w];
        *denom = s;
    }
}

// ---- Adam over a list of tensors in one launch -------------------------------------------------------------------
constexpr int ADAM_CHUNK = 2048;      // elements per block
struct AdamList {
    pn_adam_tensor t[PN_ADAM_MAX_TENSORS];
    int block_begin[PN_ADAM_MAX_TENSORS + 1];
    int n;
    float lr_over_bc1, inv_sqrt_bc2, beta1, beta2, eps, weight_decay;
    float lr;
    const pn_step_state *dyn;     // step count in device memory (hipGraph replay): the bias corrections are formed here
    int advance;                  // pn_adam_step_advance, last launch: the workgroup that finishes last moves *dyn to the next step
};

using pn::advance_step_state;      // pn_step_state.h
__global__ void adam_advance_only_kernel(pn_step_state *s) {
    if (threadIdx.x == 0 && blockIdx.x == 0) advance_step_state(s);
}

__global__ __launch_bounds__(256) void adam_kernel(AdamList a) {
    float lr_over_bc1 = a.lr_over_bc1, inv_sqrt_bc2 = a.inv_sqrt_bc2;
    if (a.dyn) {      // block-uniform: beta^step by squaring (exact enough in double; step < 2^31)
        long long n = a.dyn->adam_step;
        double p1 = 1.0, p2 = 1.0, b1 = (double)a.beta1, b2 = (double)a.beta2;
        while (n > 0) {
            if (n & 1) {
                p1 *= b1;
                p2 *= b2;
            }
            b1 *= b1;
            b2 *= b2;
            n >>= 1;
        }
        lr_over_bc1 = (float)((double)a.lr / (1.0 - p1));
        inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - p2));
    }
    int k = 0;
    while (k + 1 < a.n && (int)blockIdx.x >= a.block_begin[k + 1]) k++;      // block-uniform
    const pn_adam_tensor t = a.t[k];
    const int64_t base = (int64_t)((int)blockIdx.x - a.block_begin[k]) * ADAM_CHUNK;
    for (int i = threadIdx.x; i < ADAM_CHUNK; i += 256) {
        const int64_t e = base + i;
        if (e >= t.count) break;
        // torch/optim/adam.py (_single_tensor_adam): L2 weight decay folded into the gradient, bias-corrected
        float g = t.grad[e];
        const float p = t.param[e];
        g += a.weight_decay * p;
        const float m = a.beta1 * t.exp_avg[e] + (1.0f - a.beta1) * g;
        const float v = a.beta2 * t.exp_avg_sq[e] + (1.0f - a.beta2) * g * g;
        t.exp_avg[e] = m;
        t.exp_avg_sq[e] = v;
        t.param[e] = p - lr_over_bc1 * (m / (sqrtf(v) * inv_sqrt_bc2 + a.eps));
    }
    if (a.dyn && a.advance) {       // (block-uniform) every workgroup has read adam_step by the time it takes its ticket
        __syncthreads();
        if (threadIdx.x == 0) {
            pn_step_state *s = const_cast<pn_step_state *>(a.dyn);
            unsigned int *ticket = reinterpret_cast<unsigned int *>(&s->reserved);
            if (atomicAdd(ticket, 1u) == gridDim.x - 1) {
                atomicExch(ticket, 0u);
                advance_step_state(s);
            }
        }
    }
}

}  // namespace

namespace pn {
// loss[0] += scale * sum over rows of (logsumexp - logit[target]);  g_logits = (softmax - onehot) * scale
int launch_cross_entropy(const float *logits, const int64_t *target, int rows, int classes, float scale, float *loss,
                         float *g_logits, void *stream_, bool overwrite, const LossOpts *opts) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (rows < 1) return PN_OK;
    // Up to CE_ONE_BLOCK_ROWS rows one workgroup of 1024 threads walks them all (a few microseconds) and the loss is a
    // fixed-order sum: the same bits on every run.  Beyond that the workgroups add their parts with an atomic -- the
    // reported loss may then differ in its last bit from run to run; g_logits never does (row-wise).
    constexpr int CE_ONE_BLOCK_ROWS = 32768;
    const int threads = rows <= CE_ONE_BLOCK_ROWS ? 1024 : 256;
    const int blocks = rows <= CE_ONE_BLOCK_ROWS ? 1 : ((rows + 255) / 256 < 256 ? (rows + 255) / 256 : 256);
    if (overwrite && blocks > 1) PN_CHECK_HIP(hipMemsetAsync(loss, 0, sizeof(float), stream));
    if (opts)
        hipLaunchKernelGGL(cross_entropy_opts_kernel, dim3(blocks), dim3(threads), 0, stream, logits, target, rows, classes,
                           *opts, loss, g_logits, overwrite && blocks == 1 ? 1 : 0);
    else
        hipLaunchKernelGGL(cross_entropy_kernel, dim3(blocks), dim3(threads), 0, stream, logits, target, rows, classes, scale,
                           loss, g_logits, overwrite && blocks == 1 ? 1 : 0);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int loss_opts_from_spec(const pn_loss_spec *spec, const char *who, LossOpts *opts) {
    if (!spec) PN_FAIL(PN_ERR_ARG, "%s: null loss spec", who);
    if (!(spec->label_smoothing >= 0.0f && spec->label_smoothing <= 1.0f))
        PN_FAIL(PN_ERR_ARG, "%s: label_smoothing %g outside [0, 1]", who, (double)spec->label_smoothing);
    if (spec->reduction != PN_LOSS_MEAN && spec->reduction != PN_LOSS_SUM)
        PN_FAIL(PN_ERR_ARG, "%s: reduction %d is neither PN_LOSS_MEAN nor PN_LOSS_SUM", who, (int)spec->reduction);
    if (spec->reduction == PN_LOSS_MEAN && !spec->denominator)
        PN_FAIL(PN_ERR_ARG, "%s: the mean reduction needs a denominator", who);
    *opts = LossOpts{spec->weight, spec->denominator, spec->ignore_index, spec->has_ignore != 0 ? 1 : 0, spec->label_smoothing,
                     spec->reduction == PN_LOSS_MEAN ? 1 : 0, spec->grad_scale};
    return PN_OK;
}

int launch_loss_denominator(const int64_t *target, int rows, int classes, const LossOpts &opts, float *denom, void *stream_) {
    hipLaunchKernelGGL(loss_denominator_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream_), target, rows,
                       classes, opts, denom);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}
}  // namespace pn

extern "C" {

int pn_cross_entropy(const float *logits, const int64_t *target, int32_t rows, int32_t classes, float *loss,
                     float *g_logits, void *stream_) {
    if (!logits || !target || !loss) PN_FAIL(PN_ERR_ARG, "pn_cross_entropy: null argument");
    if (rows < 1 || classes < 1) PN_FAIL(PN_ERR_ARG, "pn_cross_entropy: rows=%d classes=%d", rows, classes);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    return pn::launch_cross_entropy(logits, target, rows, classes, 1.0f / (float)rows, loss, g_logits, stream, true);
}

int pn_loss_denominator(const int64_t *target, int32_t rows, int32_t classes, const pn_loss_spec *spec, void *stream) {
    pn::LossOpts o;
    if (int rc = pn::loss_opts_from_spec(spec, "pn_loss_denominator", &o)) return rc;
    if (!target || !spec->denominator) PN_FAIL(PN_ERR_ARG, "pn_loss_denominator: null target / denominator");
    if (rows < 1 || classes < 1) PN_FAIL(PN_ERR_ARG, "pn_loss_denominator: rows=%d classes=%d", rows, classes);
    return pn::launch_loss_denominator(target, rows, classes, o, spec->denominator, stream);
}

int pn_cross_entropy_ex(const float *logits, const int64_t *target, int32_t rows, int32_t classes, const pn_loss_spec *spec,
                        float *loss, float *g_logits, void *stream) {
    pn::LossOpts o;
    if (int rc = pn::loss_opts_from_spec(spec, "pn_cross_entropy_ex", &o)) return rc;
    if (!logits || !target || !loss) PN_FAIL(PN_ERR_ARG, "pn_cross_entropy_ex: null argument");
    if (rows < 1 || classes < 1) PN_FAIL(PN_ERR_ARG, "pn_cross_entropy_ex: rows=%d classes=%d", rows, classes);
    if (spec->denominator && !spec->denominator_given)
        if (int rc = pn::launch_loss_denominator(target, rows, classes, o, spec->denominator, stream)) return rc;
    return pn::launch_cross_entropy(logits, target, rows, classes, 0.0f, loss, g_logits, stream, true, &o);
}

static int adam_step_impl(const pn_adam_tensor *tensors, int32_t n_tensors, float lr, float beta1, float beta2, float eps,
                          float weight_decay, int64_t step, const pn_step_state *step_state, bool advance, void *stream_) {
    if (n_tensors < 0 || (n_tensors > 0 && !tensors)) PN_FAIL(PN_ERR_ARG, "pn_adam_step: bad tensor list");
    if (advance && !step_state) PN_FAIL(PN_ERR_ARG, "pn_adam_step_advance: no step state to advance");
    bool advanced = false;
    if (step_state) step = 1;       // (ignored: the kernel reads step_state->adam_step)
    if (step < 1) PN_FAIL(PN_ERR_ARG, "pn_adam_step: step counts from 1 (got %lld)", (long long)step);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const double bc1 = 1.0 - std::pow((double)beta1, (double)step), bc2 = 1.0 - std::pow((double)beta2, (double)step);
    for (int32_t at = 0; at < n_tensors; at += PN_ADAM_MAX_TENSORS) {
        AdamList a{};
        a.n = n_tensors - at < PN_ADAM_MAX_TENSORS ? n_tensors - at : PN_ADAM_MAX_TENSORS;
        int blocks = 0;
        for (int i = 0; i < a.n; i++) {
            const pn_adam_tensor &t = tensors[at + i];
            if (t.count < 0 || (t.count > 0 && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq)))
                PN_FAIL(PN_ERR_ARG, "pn_adam_step: tensor %d has a null pointer", at + i);
            a.t[i] = t;
            a.block_begin[i] = blocks;
            blocks += (int)((t.count + ADAM_CHUNK - 1) / ADAM_CHUNK);
        }
        a.block_begin[a.n] = blocks;
        a.lr_over_bc1 = (float)((double)lr / bc1);
        a.inv_sqrt_bc2 = (float)(1.0 / std::sqrt(bc2));
        a.beta1 = beta1;
        a.beta2 = beta2;
        a.eps = eps;
        a.weight_decay = weight_decay;
        a.lr = lr;
        a.dyn = step_state;
        a.advance = (advance && at + PN_ADAM_MAX_TENSORS >= n_tensors) ? 1 : 0;      // the step's last launch
        if (blocks == 0) continue;
        hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, stream, a);
        PN_CHECK_HIP(hipGetLastError());
        advanced = advanced || a.advance != 0;
    }
    if (advance && !advanced) {     // nothing to update in the last launch: the state still moves on
        hipLaunchKernelGGL(adam_advance_only_kernel, dim3(1), dim3(64), 0, stream, const_cast<pn_step_state *>(step_state));
        PN_CHECK_HIP(hipGetLastError());
    }
    return PN_OK;
}

int pn_adam_step(const pn_adam_tensor *tensors, int32_t n_tensors, float lr, float beta1, float beta2, float eps,
                 float weight_decay, int64_t step, const pn_step_state *step_state, void *stream_) {
    return adam_step_impl(tensors, n_tensors, lr, beta1, beta2, eps, weight_decay, step, step_state, false, stream_);
}

int pn_adam_step_advance(const pn_adam_tensor *tensors, int32_t n_tensors, float lr, float beta1, float beta2, float eps,
                         float weight_decay, pn_step_state *step_state, void *stream_) {
    return adam_step_impl(tensors, n_tensors, lr, beta1, beta2, eps, weight_decay, 1, step_state, true, stream_);
}

}  // extern "C"
