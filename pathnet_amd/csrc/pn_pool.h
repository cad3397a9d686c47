// pn_pool.h -- the pooling kernels of the aggregator (pn_pool.hip): attention over a node's W paths, mean, classifier -- forward,
// backward, and the training step's one launch for both with the loss in between.  Not part of the ABI.
#pragma once
#include <cstddef>
#include <cstdint>

#include "pn_internal.h"
#include "pn_loss.h"

namespace pn {

// ================================================================================================
// pool_fwd_kernel: one workgroup (4 waves) per pooling group (= output node).
// ================================================================================================
struct PoolParams {
    int variant, S, W, H, C, N;      // N: rows of Xh (sel is clamped to it, like ids in plan_kernel)
    int64_t goff;           // position of local group 0 in the whole batch (dropout counters / explicit mask rows)
    const float *hn;        // [P, H] in slot' order
    const float *ego_tab;   // Z (HOMO) or Xh (HETERO)
    const int32_t *egoidx;  // [P] row of ego_tab
    const float *Xh;        // [N, H]
    const int32_t *sel;     // [S]
    const float *att_w, *att_b, *fc2_w, *fc2_b;
    float p_drop;
    uint64_t seed;
    const pn_step_state *dyn;
    const float *mask;      // [S, 2H] or null
    float *coef;            // [P] pooling coefficient per slot' (1+att | softmax | 1)
    float *rawsc;           // [P] raw attention score (pre LeakyReLU) per slot'
    float *layer1;          // [S, 2H] classifier input after dropout
    float *out;             // [S, C]
    // optional outputs (pn_pagg_args.out_*), rows of this launch's groups; null: not written (kernel arguments: the tests
    // below are uniform over the grid -- the pooling steps, which never set them, run the same code as before)
    float *embed;           // [S, 2H] classifier input before the dropout
    float *path_weight;     // [S, W]  coef in member order
    float *path_state;      // [S, W, H] hn in member order
    // pn_path_weights.weight, or null: today's coefficients (a kernel argument too, tested uniformly over the grid).  The
    // weight of slot' is omega[slotof[slot'] - wbase]: one entry per sequence slot q of the batch, laid out like ids
    const float *omega;
    const int32_t *slotof;  // [P] the plan's slot q of every slot' of this launch
    int64_t wbase;          // first slot the caller's array holds (index_rows_local: the slice's, else 0)
    int norm;               // PN_PATH_NORM_*
};
int launch_pool_fwd(void *stream, const PoolParams &p);

// ---- pooling / attention / classifier backward: the parameters of pool_bwd_wg_kernel and of the pooling step ------------
struct PoolBwdParams {
    int variant, S, W, H, C, N;
    int64_t goff;
    const float *hn, *ego_tab;
    const int32_t *egoidx, *sel;
    const float *att_w, *fc2_w, *g_out, *coef, *rawsc;
    float p_drop;
    uint64_t seed;
    const pn_step_state *dyn;
    const float *mask;
    float *dhn;        // [P, H]
    float *dXh;        // [N, H]  (+= ego of the classifier input; HETERO: += attention ego)
    float *dego;       // table the attention-ego gradient goes to: dZ (HOMO) or dXh (HETERO)
    float *g_att_w, *g_att_b;
    // instead of atomics the kernel stores the attention-weight terms per workgroup (always) and, in deterministic mode
    // (else null), the ego half of d layer1 per group and d score per path; det_att_reduce_kernel / det_scatter_kernel add
    float *det_sel;    // [S, H]
    float *det_ds;     // [P]
    float *det_att;    // [workgroups][2H + 4]
    // pn_pagg_args.g_embed: d loss / d (classifier input before the dropout) [S, 2H] of this launch's groups, or null.  g_out
    // may be null when it is set (the classifier's term is then absent)
    const float *g_embed;
    // the path weights, as in PoolParams: coef holds kappa * omega * c already; the score gradient needs kappa, recomputed from
    // the group's W weights
    const float *omega;
    const int32_t *slotof;
    int64_t wbase;
    int norm;
    // gradients at the per-path interface (pn_path_grads), each null or set for the whole launch:
    const float *g_state;   // [S, W, H] upstream of PoolParams::path_state, rows of this launch's groups: joins d h_n
    const float *g_coef;    // [S, W]    upstream of PoolParams::path_weight: joins d coef behind the dot product
    float *d_omega;         // out, indexed like omega: d loss / d weight, 0 where the weight is not live or the group is empty;
                            // every member of every group of the launch is stored once (needs omega)
};
// HI = 4 up to H = 256, HI = 16 above
int launch_pool_bwd(pn_context *ctx, void *stream, const PoolBwdParams &p);

// LDS of the widest of the two kernels above for W walks per node at hidden size H: what a shape has to fit into 64 KiB
size_t pool_lds_bytes(int W, int H);

// ---- pooling forward, loss and pooling backward of a group in ONE launch (pn_pagg_train_step, default mode) -----------------
// Between the recurrence and the BPTT a training step has, per masked node and independent of every other node: attention +
// pooling + classifier (pool_fwd_kernel), softmax cross entropy of its C logits (cross_entropy_kernel) and the pooling /
// attention backward (pool_bwd_wg_kernel) -- three dependent launches of ~20 us each for work that touches 40 KB per node.
// One workgroup per node runs the three bodies back to back: the node's h_n and ego rows are re-read from the CU's own
// caches, the logits and their gradient never leave the workgroup's sight.  The same code as the three kernels (the
// bodies ARE those kernels'), so logits, g_out, d h_n and every gradient term are bit-identical to the three launches;
// the loss is the fixed-order sum of the per-node terms (loss_sum_kernel, off the critical path).
// Replaces /root/reference/PathNet_run.py:196-210 / :266-277 (forward), :346 (loss) and autograd's backward of both.
struct PoolStepParams {
    PoolParams f;
    PoolBwdParams b;
    const int64_t *target;  // [S] class of each group
    float scale;            // d loss / d (row loss): grad_scale / rows of the whole batch
    float *gout;            // [S, C] d loss / d logits (read by the classifier's weight-gradient GEMM)
    float *lossg;           // [S] logsumexp - logit[target] per group
};
// ---- the step with pn_loss_spec's options (pn_pagg_train_step_loss): the row is pn_loss.h's, as cross_entropy_opts_kernel
// walks it; k = grad_scale / D comes from D in device memory.  A kernel of its own: pool_step_kernel is as it was.
struct PoolStepLossParams {
    PoolStepParams s;       // (s.scale is not read: the options carry grad_scale)
    LossOpts o;
};
// The pooling step of micro-batch ps.f.S groups, with the loss options when opts is set.  knob = PN_POOL_STEP (Knobs::pool_step,
// non-zero here): the node's rows in registers (pool_step2_kernel<10, 2>) when
//     W <= 40 && 32 <= H <= 128 && its LDS <= 64 KiB && knob >= 1 && knob != 2 && no path weights (ps.f.omega null),
// else the three bodies back to back: pool_step_kernel<4> up to H = 256, <16> above.  pool_step2_kernel does not carry the
// path weights: a weighted call always takes the three bodies, an unweighted one goes exactly where it went before.
int launch_pool_step(pn_context *ctx, void *stream, const PoolStepParams &ps, const LossOpts *opts, int knob);

// loss[0] (+)= k * sum of the rows' terms lossg[0 .. rows), one workgroup, cross_entropy_kernel's order; k = scale, or with opts
// the options' grad_scale / D (mean) or grad_scale (sum), formed on the device
int launch_loss_sum(void *stream, const float *lossg, int rows, float scale, const LossOpts *opts, float *loss, bool store);

// g_att_w [2H] / g_att_b [1] += the pooling backward's per-workgroup terms (PoolBwdParams::det_att, nblk workgroups) in workgroup order
int launch_att_reduce(void *stream, const float *part, int nblk, int H, float *g_att_w, float *g_att_b);

}  // namespace pn
