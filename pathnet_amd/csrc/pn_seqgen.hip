// pn_seqgen.hip -- the path encoders beside the fused recurrent kernels (pn_seqh.hip / pn_seq3.hip) on gfx950: the
// order-agnostic mean / sum encoders of the ablation and the step-by-step recurrence for hidden sizes above 256.
// Launch parameters and launchers: pn_seq.h; the cell functions and the bias / row maps of the packing: pn_seq_core.h.
#include <hip/hip_runtime.h>

#include "pn_internal.h"
#include "pn_kernels.h"
#include "pn_seq.h"
#include "pn_seq_core.h"

using namespace pn;

namespace {

// ---- the mean / sum encoders (SeqReduceParams: pn_seq.h) ----------------------------------------------------------------
template <bool BACKWARD>
__global__ __launch_bounds__(256) void seq_reduce_kernel(SeqReduceParams p) {
    const int hv = p.H / 4;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)p.P * hv) return;
    const int q = (int)(i / hv), c4 = (int)(i - (int64_t)q * hv);
    const uint64_t seed = p.dyn ? p.dyn->seed : p.seed;
    const int64_t slot = p.slotof[q];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (BACKWARD) {
        g = reinterpret_cast<const float4 *>(p.dhn)[i];
        g.x *= p.scale; g.y *= p.scale; g.z *= p.scale; g.w *= p.scale;
    }
    for (int t = 0; t < p.L; t++) {
        float4 m = make_float4(1.f, 1.f, 1.f, 1.f);
        if (p.mask)
            m = reinterpret_cast<const float4 *>(p.mask)[((int64_t)t * p.Pmask + slot) * hv + c4];
        else if (p.p_drop > 0.0f)
            m = dropout4(seed, ((uint64_t)t * p.Pmask + slot) * hv + c4, 1u, p.p_drop);     // the recurrent kernels' counters
        const size_t row = (size_t)(uint32_t)p.rowidx[(int64_t)q * p.L + t];
        if (BACKWARD) {
            float *d = p.dZ + row * p.H + 4 * c4;
            atomicAdd(d + 0, g.x * m.x); atomicAdd(d + 1, g.y * m.y); atomicAdd(d + 2, g.z * m.z); atomicAdd(d + 3, g.w * m.w);
        } else {
            const float4 v = reinterpret_cast<const float4 *>(p.Z)[row * hv + c4];
            acc.x += v.x * m.x; acc.y += v.y * m.y; acc.z += v.z * m.z; acc.w += v.w * m.w;
        }
    }
    if (!BACKWARD) {
        acc.x *= p.scale; acc.y *= p.scale; acc.z *= p.scale; acc.w *= p.scale;
        reinterpret_cast<float4 *>(p.hn)[i] = acc;
    }
}

// ================================================================================================
// Generic recurrence for hidden sizes the fused kernels do not cover (256 < H <= 1024, e.g. the reference's -hid=1024
// runs, results/result_for_Nba.txt): step by step -- gather + dropout kernel, one fp32 MFMA GEMM for the gate
// pre-activations, an element-wise cell kernel; backward the same way round plus one GEMM for the weight gradients.
// Same tensors and layouts as the fused path (saved [P,L,SV,H], xh [P,L,2H], dG [P,L,GH]), same dropout counters, so
// pooling, micro-batches, slices and the caller see no difference.  A functional path, ~10 launches per step.
// ================================================================================================
// (GenParams: pn_seq.h)
__device__ __forceinline__ float4 gen_mask(const GenParams &p, uint64_t seed, int t, int64_t slot, int c4) {
    const int hv = p.H / 4;
    if (p.mask) return reinterpret_cast<const float4 *>(p.mask)[((int64_t)t * p.Pmask + slot) * hv + c4];
    if (p.p_drop > 0.0f) return dropout4(seed, ((uint64_t)t * p.Pmask + slot) * hv + c4, 1u, p.p_drop);
    return make_float4(1.f, 1.f, 1.f, 1.f);
}

// xh[q, t, 0:H] = mask * Z[row(q, t)];  t = 0 also clears the h half
__global__ __launch_bounds__(256) void gen_x_kernel(GenParams p) {
    const int hv = p.H / 4;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)p.P * hv) return;
    const int q = (int)(i / hv), c4 = (int)(i - (int64_t)q * hv);
    const uint64_t seed = p.dyn ? p.dyn->seed : p.seed;
    const float4 m = gen_mask(p, seed, p.t, p.slotof[q], c4);
    const size_t row = (size_t)(uint32_t)p.rowidx[(int64_t)q * p.L + p.t];
    float4 v = reinterpret_cast<const float4 *>(p.Z)[row * hv + c4];
    v.x *= m.x; v.y *= m.y; v.z *= m.z; v.w *= m.w;
    float4 *dst = reinterpret_cast<float4 *>(p.xh) + ((size_t)q * p.L + p.t) * (2 * hv) + c4;
    dst[0] = v;
    if (p.t == 0) dst[hv] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// one element (path q, hidden unit j) of the cell update of step t
__global__ __launch_bounds__(256) void gen_cell_fwd_kernel(GenParams p) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)p.P * p.H) return;
    const int H = p.H, q = (int)(i / H), j = (int)(i - (int64_t)q * H);
    const float *pre = p.pre + ((size_t)q * p.L + p.t) * ((size_t)p.G * H) + j;
    const int SV = p.G == 4 ? 5 : 1;
    float *sv = p.saved ? p.saved + (((size_t)q * p.L + p.t) * SV) * H + j : nullptr;
    float h;
    if (p.cell == 3) {                     // GRU on the four slots r, z, nx, nh
        const float pr = pre[0], pz = pre[H], pnh = pre[3 * (size_t)H], pnx = pre[2 * (size_t)H];
        const float hp = p.t > 0 ? p.state[i] : 0.0f;
        const GruFwd c = gru_fwd(pr, pz, pnx, pnh, hp);
        h = c.h;
        p.state[i] = h;
        if (sv) { sv[0] = c.rg; sv[H] = c.zg; sv[2 * (size_t)H] = c.ng; sv[3 * (size_t)H] = c.nh; sv[4 * (size_t)H] = hp; }
    } else if (p.G == 4) {                 // LSTM
        const LstmFwd c = lstm_fwd(pre[0], pre[H], pre[2 * (size_t)H], pre[3 * (size_t)H], p.t > 0 ? p.state[i] : 0.0f);
        p.state[i] = c.c;
        h = c.h;
        if (sv) { sv[0] = c.ig; sv[H] = c.fg; sv[2 * (size_t)H] = c.gg; sv[3 * (size_t)H] = c.og; sv[4 * (size_t)H] = c.c; }
    } else {                                // tanh RNN
        h = rnn_fwd(pre[0]);
        if (sv) sv[0] = h;
    }
    if (p.t == p.L - 1)
        p.hn[i] = h;
    else
        p.xh[((size_t)q * p.L + p.t + 1) * (2 * (size_t)H) + H + j] = h;
}

// cell backward of step t: dh (in place buffer) and the carried state -> the gate-slot gradients dG[q, t, :]
__global__ __launch_bounds__(256) void gen_cell_bwd_kernel(GenParams p) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)p.P * p.H) return;
    const int H = p.H, q = (int)(i / H), j = (int)(i - (int64_t)q * H);
    const int SV = p.G == 4 ? 5 : 1;
    const float *sv = p.saved + (((size_t)q * p.L + p.t) * SV) * H + j;
    float *d = p.pre + ((size_t)q * p.L + p.t) * ((size_t)p.G * H) + j;
    const float dhv = p.dh[i];
    if (p.cell == 3) {
        const float rg = sv[0], zg = sv[H], ng = sv[2 * (size_t)H], nh = sv[3 * (size_t)H], hp = sv[4 * (size_t)H];
        const CellGrad c = gru_bwd(rg, zg, ng, nh, hp, dhv, true);
        d[0] = c.a0; d[H] = c.a1; d[2 * (size_t)H] = c.a2; d[3 * (size_t)H] = c.a3;
        p.state[i] = c.carry;               // the direct path d h_t / d h_{t-1}
    } else if (p.G == 4) {
        const float ig = sv[0], fg = sv[H], gg = sv[2 * (size_t)H], og = sv[3 * (size_t)H], ct = sv[4 * (size_t)H];
        const float cprev = p.t > 0 ? sv[-(ptrdiff_t)H] : 0.0f;       // slot 4 of step t-1
        const CellGrad c = lstm_bwd(ig, fg, gg, og, cprev, ct, dhv, p.t < p.L - 1 ? p.state[i] : 0.0f, true);
        d[0] = c.a0; d[H] = c.a1; d[2 * (size_t)H] = c.a2; d[3 * (size_t)H] = c.a3;
        p.state[i] = c.carry;
    } else {
        d[0] = rnn_bwd(sv[0], dhv, true);
    }
}

// after the step's GEMM gx = dG_t . [W_ih | W_hh]: scatter mask * dx into dZ, dh_{t-1} into the dh buffer
__global__ __launch_bounds__(256) void gen_scatter_kernel(GenParams p) {
    const int hv = p.H / 4;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)p.P * hv) return;
    const int q = (int)(i / hv), c4 = (int)(i - (int64_t)q * hv);
    const uint64_t seed = p.dyn ? p.dyn->seed : p.seed;
    const float4 m = gen_mask(p, seed, p.t, p.slotof[q], c4);
    const float4 *g = reinterpret_cast<const float4 *>(p.gx) + (size_t)q * (2 * hv) + c4;
    const float4 dx = g[0];
    const size_t row = (size_t)(uint32_t)p.rowidx[(int64_t)q * p.L + p.t];
    float *dz = p.dZ + row * p.H + 4 * c4;
    atomicAdd(dz + 0, dx.x * m.x); atomicAdd(dz + 1, dx.y * m.y); atomicAdd(dz + 2, dx.z * m.z); atomicAdd(dz + 3, dx.w * m.w);
    if (p.t > 0) {
        float4 dh = g[hv];
        if (p.cell == 3) {
            const float4 direct = reinterpret_cast<const float4 *>(p.state)[i];
            dh.x += direct.x; dh.y += direct.y; dh.z += direct.z; dh.w += direct.w;
        }
        reinterpret_cast<float4 *>(p.dh)[i] = dh;
    }
}

// Wcat [GH, 2H] = [W_ih | W_hh] in fp32 (GRU: the four slots with their zero halves) and its transpose, biasc as in
// the fused kernels' packings (packed_bias)
__global__ void gen_pack_kernel(const float *__restrict__ w_ih, const float *__restrict__ w_hh,
                                const float *__restrict__ b_ih, const float *__restrict__ b_hh, int H, int G, int gru,
                                float *__restrict__ Wcat, float *__restrict__ WcatT, float *__restrict__ biasc) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (int64_t)G * H) biasc[i] = packed_bias(b_ih, b_hh, i, H, gru);
    if (i >= (int64_t)G * H * 2 * H) return;
    const int m = (int)(i / (2 * H)), k = (int)(i - (int64_t)m * 2 * H), slot = m / H, j = m - slot * H;
    const int row = gru ? gru_weight_row(slot, j, H) : m;
    float v = k < H ? w_ih[(int64_t)row * H + k] : w_hh[(int64_t)row * H + (k - H)];
    if (gru && ((slot == 2 && k >= H) || (slot == 3 && k < H))) v = 0.0f;
    Wcat[i] = v;
    if (WcatT) WcatT[(int64_t)k * G * H + m] = v;      // [2H, GH]: the BPTT's GEMM wants its B operand K-contiguous too
}

}  // namespace

namespace pn {

int launch_seq_reduce(void *stream, const SeqReduceParams &p, bool backward) {
    const int64_t n = (int64_t)p.P * (p.H / 4);
    if (backward)
        hipLaunchKernelGGL(seq_reduce_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(seq_reduce_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

// a thread per (path, 4 columns): gen_x / gen_scatter; a thread per (path, hidden unit): the cell kernels
static inline unsigned gen_blocks4(const GenParams &p) { return (unsigned)(((int64_t)p.P * (p.H / 4) + 255) / 256); }
static inline unsigned gen_blocks1(const GenParams &p) { return (unsigned)(((int64_t)p.P * p.H + 255) / 256); }

int launch_gen_x(void *stream, const GenParams &p) {
    hipLaunchKernelGGL(gen_x_kernel, dim3(gen_blocks4(p)), dim3(256), 0, (hipStream_t)stream, p);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int launch_gen_cell_fwd(void *stream, const GenParams &p) {
    hipLaunchKernelGGL(gen_cell_fwd_kernel, dim3(gen_blocks1(p)), dim3(256), 0, (hipStream_t)stream, p);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int launch_gen_cell_bwd(void *stream, const GenParams &p) {
    hipLaunchKernelGGL(gen_cell_bwd_kernel, dim3(gen_blocks1(p)), dim3(256), 0, (hipStream_t)stream, p);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int launch_gen_scatter(void *stream, const GenParams &p) {
    hipLaunchKernelGGL(gen_scatter_kernel, dim3(gen_blocks4(p)), dim3(256), 0, (hipStream_t)stream, p);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int launch_gen_pack(void *stream, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, int H, int G, int gru,
                    float *Wcat, float *WcatT, float *biasc) {
    const int64_t n = (int64_t)G * H * 2 * H;
    hipLaunchKernelGGL(gen_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w_ih, w_hh, b_ih, b_hh,
                       H, G, gru, Wcat, WcatT, biasc);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

}  // namespace pn
