// pn_loss.h -- the loss options (pn_loss_spec: class weights, ignore_index, label smoothing) as the kernels take them, and
// the one row of the option-aware softmax cross entropy that pn_train.hip's stand-alone kernel and pn_pool.hip's fused
// pooling step (pool_step_loss_kernel) share -- the same lines, hence the same bits on both routes.
// The arithmetic is written out above pn_loss_spec in include/pathnet_hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace pn {

struct LossOpts {           // pn_loss_spec, checked (loss_opts_from_spec, pn_train.hip)
    const float *weight;    // dev [C] or null: all ones
    const float *denom;     // dev float D, read when the kernel runs (null with the sum reduction)
    int64_t ignore;
    int has_ignore;
    float eps;              // label smoothing
    int mean;               // 1: k = grad_scale / D, 0: k = grad_scale
    float grad_scale;
};

// k for the gradients and k for the loss.  D == 0 (or NaN) under the mean: zero gradients, NaN loss
__device__ __forceinline__ void loss_factors(const LossOpts &o, float &k_grad, float &k_loss) {
    if (!o.mean) {
        k_grad = k_loss = o.grad_scale;
        return;
    }
    const float D = *o.denom;
    const bool ok = fabsf(D) > 0.0f;
    const float k = o.grad_scale / D;
    k_grad = ok ? k : 0.0f;
    k_loss = ok ? k : NAN;
}

// One row, walked by one thread as cross_entropy_kernel walks it: returns the row's loss term l_r (0 for an ignored row, NaN
// for a target outside [0, classes) that is not the ignore value) and writes d loss / d logits to g (or null) -- exact zeros
// for both kinds of dropped row.  No address is formed from the target unchecked: a clamped index and selects, and the
// selects also keep an ignored row's logits (which may be NaN) out of everything.
// With every option off the terms reduce to cross_entropy_kernel's, bit for bit: a = 1 multiplies exactly.
__device__ __forceinline__ float ce_row_opts(const float *__restrict__ x, int classes, int64_t t64, const LossOpts &o,
                                             float k_grad, float *__restrict__ g) {
    const bool ign = o.has_ignore && t64 == o.ignore;
    const bool ok = t64 >= 0 && t64 < (int64_t)classes;
    const bool kept = ok && !ign;
    const int t = ok ? (int)t64 : 0;
    float m = x[0];
    for (int c = 1; c < classes; c++) m = fmaxf(m, x[c]);
    float s = 0.0f;
    for (int c = 0; c < classes; c++) s += expf(x[c] - m);
    const float ls = logf(s);
    const float a = (1.0f - o.eps) * (o.weight ? o.weight[t] : 1.0f);
    float row = a * (ls - (x[t] - m));
    const bool smooth = o.eps != 0.0f;
    const float es = o.eps / (float)classes;
    float wsum = 0.0f;
    if (smooth) {
        float sm = 0.0f;
        for (int c = 0; c < classes; c++) {
            const float wc = o.weight ? o.weight[c] : 1.0f;
            sm += wc * (ls - (x[c] - m));
            wsum += wc;
        }
        row += es * sm;
    }
    if (g) {
        for (int c = 0; c < classes; c++) {
            const float p = expf((x[c] - m) - ls);
            float gv = ((p - (c == t ? 1.0f : 0.0f)) * a) * k_grad;
            if (smooth) gv += (es * (wsum * p - (o.weight ? o.weight[c] : 1.0f))) * k_grad;
            g[c] = kept ? gv : 0.0f;
        }
    }
    return ign ? 0.0f : (ok ? row : NAN);
}

}  // namespace pn
