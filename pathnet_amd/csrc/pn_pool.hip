// pn_pool.hip -- the pooling kernels of the aggregator on gfx950: attention over the W paths of a node, mean, concat ego,
// dropout, fc2 (pool_fwd_kernel), their backward (pool_bwd_wg_kernel), the training step's fusion of both with the loss in
// between (pool_step_kernel, pool_step2_kernel and their loss-option twins), and the two fixed-order finishes behind them
// (loss_sum_kernel, det_att_reduce_kernel).  Every LDS byte count stands right behind the kernel whose carving it restates.
// Launch parameters and launchers: pn_pool.h.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pn_internal.h"
#include "pn_kernels.h"
#include "pn_loss.h"
#include "pn_pool.h"

using namespace pn;

namespace {

// ---- path weights (pn_path_weights; PoolParams::omega) ---------- ----------------------------------------------------------
// a weight that is no finite positive number counts as 0 (bit test: positive, non-zero, below +inf)
__device__ __forceinline__ float live_weight(float w) { return (__float_as_uint(w) - 1u) < 0x7f7fffffu ? w : 0.0f; }
// kappa of a group from its W live weights in LDS: W / sum (PN_PATH_NORM_SUM) or 1 (PN_PATH_NORM_COUNT); 0 for an empty group,
// and for a sum so small that W / sum leaves fp32.  Every wave adds all W in the same order: the same value in each; W ones
// add up to W exactly, so all-one weights give exactly 1.
__device__ __forceinline__ float pool_kappa(const float *s_om, int W, int norm, int lane) {
    float om = 0.0f;
    for (int mem = lane; mem < W; mem += 64) om += s_om[mem];
    om = wave_sum(om);
    if (norm == PN_PATH_NORM_COUNT) return om > 0.0f ? 1.0f : 0.0f;
    const float k = (float)W / om;
    return k < 3.0e38f ? k : 0.0f;
}

// (PoolParams: pn_pool.h)
__device__ __forceinline__ void pool_fwd_body(const PoolParams &p, float *lds) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int g = blockIdx.x, H = p.H, W = p.W;
    float *sc = lds;                                            // [W] scores, then coefficients
    int *s_erow = reinterpret_cast<int *>(sc + W);              // [W] ego rows of the group's members
    float *part4 = reinterpret_cast<float *>(s_erow + W);       // [4][H] the waves' partial pooled sums
    float *l1s = part4 + 4 * H;                                 // [2H] classifier input
    float *s_om = l1s + 2 * H;                                  // [W] live path weights (with p.omega)
    const float inv_w = 1.0f / (float)W;
    // without weights every factor below is the constant 1: x * 1 is x, the coefficients keep their bits
    float kappa = 1.0f;
    if (p.omega) {
        for (int mem = tid; mem < W; mem += 256)
            s_om[mem] = live_weight(p.omega[(int64_t)p.slotof[(int64_t)g * W + mem] - p.wbase]);
        __syncthreads();
        kappa = pool_kappa(s_om, W, p.norm, lane);
    }
    auto om = [&](int mem) { return p.omega ? s_om[mem] : 1.0f; };

    if (p.variant != PN_VARIANT_PAGG) {
        // the ego rows, fetched up front: the score loop then has no index -> row dependent load pair
        for (int mem = tid; mem < W; mem += 256) s_erow[mem] = p.egoidx[(int64_t)g * W + mem];
        __syncthreads();
        // attention scores, 8 members per wave at a time: lane = (member lane>>3, eighth of H lane&7); the eight partial
        // dot products of a member are summed with three xor-shuffles
        const float ab = p.att_b[0];
        const int m8 = lane >> 3, part = lane & 7, jw = H / 8;
        for (int m0 = 8 * wave; m0 < W; m0 += 32) {
            const int mem = m0 + m8;
            const int memc = min(mem, W - 1);
            const int64_t s = (int64_t)g * W + memc;
            const float4 *h4 = reinterpret_cast<const float4 *>(p.hn + s * H + part * jw);
            const float4 *e4 = reinterpret_cast<const float4 *>(p.ego_tab + (int64_t)s_erow[memc] * H + part * jw);
            const float4 *a4 = reinterpret_cast<const float4 *>(p.att_w + part * jw);
            const float4 *b4 = reinterpret_cast<const float4 *>(p.att_w + H + part * jw);
            float acc = 0.0f;
            for (int j = 0; j < jw / 4; j++) {
                const float4 hv = h4[j], ev = e4[j], av = a4[j], bv = b4[j];
                acc += hv.x * av.x + hv.y * av.y + hv.z * av.z + hv.w * av.w;
                acc += ev.x * bv.x + ev.y * bv.y + ev.z * bv.z + ev.w * bv.w;
            }
            acc += __shfl_xor(acc, 1, 64);
            acc += __shfl_xor(acc, 2, 64);
            acc += __shfl_xor(acc, 4, 64);
            if (part == 0 && mem < W) {
                sc[mem] = acc + ab;
                p.rawsc[(int64_t)g * W + mem] = acc + ab;
            }
        }
        __syncthreads();
    }
    if (p.variant == PN_VARIANT_HETERO) {
        // softmax over the W members of LeakyReLU(score) (F.softmax implicit dim 0 of [W,S,1]); every wave reduces
        // all W scores (same order, same result), then each thread rewrites its own entries
        float mx = -3.4e38f;
        for (int mem = lane; mem < W; mem += 64) {
            float v = sc[mem];
            v = v > 0.0f ? v : 0.01f * v;
            mx = fmaxf(mx, v);
        }
        mx = wave_max(mx);
        float sum = 0.0f;
        for (int mem = lane; mem < W; mem += 64) {
            float v = sc[mem];
            v = v > 0.0f ? v : 0.01f * v;
            sum += om(mem) * expf(v - mx);
        }
        sum = wave_sum(sum);
        __syncthreads();
        // (the maximum is over all members, live or not; a group whose live members' terms sum to 0 pools nothing)
        for (int mem = tid; mem < W; mem += 256) {
            float v = sc[mem];
            v = v > 0.0f ? v : 0.01f * v;
            sc[mem] = (!p.omega || sum > 0.0f) ? kappa * (om(mem) * expf(v - mx) / sum) : 0.0f;
        }
    } else if (p.variant == PN_VARIANT_HOMO) {
        for (int mem = tid; mem < W; mem += 256) sc[mem] = (kappa * om(mem)) * (1.0f + sc[mem]);
    } else {
        for (int mem = tid; mem < W; mem += 256) sc[mem] = kappa * om(mem);
    }
    __syncthreads();
    for (int mem = tid; mem < W; mem += 256) p.coef[(int64_t)g * W + mem] = sc[mem];
    if (p.path_weight)
        for (int mem = tid; mem < W; mem += 256) p.path_weight[(int64_t)g * W + mem] = sc[mem];
    if (p.path_state) {     // the group's W rows of hn are already in member order: one contiguous copy (H % 32 == 0)
        const float4 *src = reinterpret_cast<const float4 *>(p.hn + (int64_t)g * W * H);
        float4 *dst = reinterpret_cast<float4 *>(p.path_state + (int64_t)g * W * H);
        for (int i = tid; i < W * H / 4; i += 256) dst[i] = src[i];
    }

    // pooled = mean_w coef_w * h_w: each wave sums its quarter of the members, the quarters meet in LDS (fixed order)
    {
        const int per = (W + 3) / 4, mem_end = min(W, (wave + 1) * per);
        for (int j = lane; j < H; j += 64) {
            float acc = 0.0f;
#pragma unroll 8
            for (int mem = wave * per; mem < mem_end; mem++) acc += sc[mem] * p.hn[((int64_t)g * W + mem) * H + j];
            part4[wave * H + j] = acc;
        }
    }
    __syncthreads();
    // layer1 = dropout([Xh[sel[g]] ; pooled])
    float *l1 = p.layer1 + (int64_t)g * 2 * H;
    const float *ego = p.Xh + (int64_t)min(max(p.sel[g], 0), p.N - 1) * H;
    for (int j = tid; j < H; j += 256) {
        float a = ego[j], b = (part4[j] + part4[H + j] + part4[2 * H + j] + part4[3 * H + j]) * inv_w;
        if (p.embed) {
            p.embed[(int64_t)g * 2 * H + j] = a;
            p.embed[(int64_t)g * 2 * H + H + j] = b;
        }
        const uint64_t gg = (uint64_t)(p.goff + g);
        if (p.mask) {
            a *= p.mask[gg * 2 * H + j];
            b *= p.mask[gg * 2 * H + H + j];
        } else if (p.p_drop > 0.0f) {
            const uint64_t seed = p.dyn ? p.dyn->seed : p.seed;
            const float4 m0 = dropout4(seed, (gg * 2 * H + j) >> 2, 2u, p.p_drop);
            const float4 m1 = dropout4(seed, (gg * 2 * H + H + j) >> 2, 2u, p.p_drop);
            const int e0 = j & 3;
            a *= e0 == 0 ? m0.x : e0 == 1 ? m0.y : e0 == 2 ? m0.z : m0.w;
            b *= e0 == 0 ? m1.x : e0 == 1 ? m1.y : e0 == 2 ? m1.z : m1.w;
        }
        l1[j] = a;
        l1[H + j] = b;
        l1s[j] = a;
        l1s[H + j] = b;
    }
    __syncthreads();
    for (int c = wave; c < p.C; c += 4) {
        float part = 0.0f;
        for (int j = lane; j < 2 * H; j += 64) part += l1s[j] * p.fc2_w[(int64_t)c * 2 * H + j];
        part = wave_sum(part);
        if (lane == 0) p.out[(int64_t)g * p.C + c] = part + p.fc2_b[c];
    }
}
__global__ __launch_bounds__(256) void pool_fwd_kernel(PoolParams p) {
    extern __shared__ float lds[];
    pool_fwd_body(p, lds);
}
inline size_t pool_fwd_lds_bytes(int W, int H) { return (3 * (size_t)W + 6 * (size_t)H) * sizeof(float); }

// ================================================================================================
// BACKWARD
// ================================================================================================
// (PoolBwdParams: pn_pool.h)
// A workgroup per group: the W members of a group split over the four waves.  (A wavefront per group ran its ~50 dependent
// memory round trips alone on its SIMD -- 1 299 waves on 1 024 SIMDs at the headline shape; four times the waves hide them:
// 0.052 -> 0.031 ms.  Round 2 had rejected this layout for quadrupling the atomics on the 2H + 1 attention-weight
// addresses; those go through per-workgroup partials, det_att: [groups][2H + 4].)
// HI: 64-column chunks of H a lane walks (4 covers H <= 256, the fused kernels' range; 16 covers the generic path's H <= 1024)
template <int HI>
__device__ __forceinline__ void pool_bwd_wg_body(const PoolBwdParams &p, float *lds) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int H = p.H, W = p.W;
    float *dco = lds;                        // [W] d coef
    float *dsc = dco + W;                    // [W] d score
    float *dp = dsc + W;                     // [H] d pooled / W
    float *red = dp + H;                     // [4][2H] per-wave attention-weight partials; before that [4][H] ego partials
    int *s_erow = reinterpret_cast<int *>(red + 8 * H);    // [W] ego rows of the group
    float *s_coef = reinterpret_cast<float *>(s_erow + W);  // [W]
    float *s_tot = s_coef + W;               // [4] hetero: partial sums of coef * d coef
    float *s_kw = s_tot + 4;                 // [W] live path weights (with p.omega; pool_bwd_lds_bytes has the room)
    int *s_slot = reinterpret_cast<int *>(s_kw + W);       // [W] their entries of omega / d_omega (5 W + 9 H + 4 words so far of 16 W + 12 H)
    const int g = blockIdx.x;
    const float inv_w = 1.0f / (float)W;
    for (int mem = tid; mem < W; mem += 256) {
        const int64_t s = (int64_t)g * W + mem;
        s_erow[mem] = p.variant == PN_VARIANT_PAGG ? 0 : p.egoidx[s];
        s_coef[mem] = p.coef[s];
    }
    if (p.omega)        // (a loop of its own: inside the one above it costs pool_bwd_wg_kernel<4> 22 registers)
        for (int mem = tid; mem < W; mem += 256) {
            const int64_t q = (int64_t)p.slotof[(int64_t)g * W + mem] - p.wbase;
            s_kw[mem] = live_weight(p.omega[q]);
            s_slot[mem] = (int)q;       // (d_omega's index, kept here: formed again at its store it costs the <4> kernel 24 registers)
        }
    for (int j = tid; j < H; j += 256) {
        float a = 0.0f, b = 0.0f;
        if (p.g_out)
            for (int c = 0; c < p.C; c++) {
                const float go = p.g_out[(int64_t)g * p.C + c];
                a += go * p.fc2_w[(int64_t)c * 2 * H + j];
                b += go * p.fc2_w[(int64_t)c * 2 * H + H + j];
            }
        const uint64_t gg = (uint64_t)(p.goff + g);
        if (p.mask) {
            a *= p.mask[gg * 2 * H + j];
            b *= p.mask[gg * 2 * H + H + j];
        } else if (p.p_drop > 0.0f) {
            const uint64_t seed = p.dyn ? p.dyn->seed : p.seed;
            a *= dropout1(seed, gg * 2 * H + j, 2u, p.p_drop);
            b *= dropout1(seed, gg * 2 * H + H + j, 2u, p.p_drop);
        }
        if (p.g_embed) {    // the embedding is read before the dropout: its gradient joins behind the mask
            a += p.g_embed[(int64_t)g * 2 * H + j];
            b += p.g_embed[(int64_t)g * 2 * H + H + j];
        }
        if (p.det_sel)
            p.det_sel[(int64_t)g * H + j] = a;
        else
            atomicAdd(&p.dXh[(int64_t)min(max(p.sel[g], 0), p.N - 1) * H + j], a);
        dp[j] = b * inv_w;
    }
    __syncthreads();
    {       // d coef[mem] = hn[mem] . d pooled / W: eight lanes per member, 32 members per pass
        const int m32 = tid >> 3, part = tid & 7, jw = H / 8;
        for (int m0 = 0; m0 < W; m0 += 32) {
            const int mem = m0 + m32;
            const float4 *h4 = reinterpret_cast<const float4 *>(p.hn + ((int64_t)g * W + min(mem, W - 1)) * H + part * jw);
            float acc = 0.0f;
            for (int j = 0; j < jw / 4; j++) {
                const float4 hv = h4[j];
                const float *d = dp + part * jw + 4 * j;
                acc += hv.x * d[0] + hv.y * d[1] + hv.z * d[2] + hv.w * d[3];
            }
            acc += __shfl_xor(acc, 1, 64);
            acc += __shfl_xor(acc, 2, 64);
            acc += __shfl_xor(acc, 4, 64);
            if (part == 0 && mem < W) dco[mem] = p.g_coef ? acc + p.g_coef[(int64_t)g * W + mem] : acc;
        }
    }
    __syncthreads();
    // coef = kappa * omega * c: d score = kappa * omega * d coef (HOMO), and the softmax's sum carries 1 / kappa (HETERO: with
    // coef = kappa * a, d l_m = coef_m * (d coef_m - sum_k coef_k d coef_k / kappa)).  Without weights both factors are 1.
    const float kappa = p.omega ? pool_kappa(s_kw, W, p.norm, lane) : 1.0f;
    if (p.d_omega) {
#pragma clang fp contract(off)      // (an fma of the last difference would keep one product's rounding error)
        // d loss / d w_j of the live weights, D = d coef above (g_coef included), T = sum coef D, Om = sum w:
        //   PAGG / HOMO  (coef_j D_j Om - [sum] w_j T) / (w_j Om)         HETERO  (coef_j (D_j - T / kappa) Om - [sum] w_j T) / (w_j Om)
        // ([sum]: PN_PATH_NORM_SUM only, kappa's own derivative).  T, Om and the differences in fp64 -- W scalar operations: a
        // group with one live path under "sum" is scale invariant, and (coef_j D_j) w_j - w_j (coef_j D_j) is 0 exactly.  Every
        // wave adds all W in the same order; every member is stored, the dead ones and an empty group's as 0
        double T = 0.0, Om = 0.0;
        for (int mem = lane; mem < W; mem += 64) {
            T += (double)s_coef[mem] * (double)dco[mem];
            Om += (double)s_kw[mem];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            T += __shfl_xor(T, o, 64);
            Om += __shfl_xor(Om, o, 64);
        }
        const double Tk = (p.variant == PN_VARIANT_HETERO && kappa > 0.0f) ? T / (double)kappa : 0.0;
        const double To = p.norm == PN_PATH_NORM_SUM ? T : 0.0;
        for (int mem = tid; mem < W; mem += 256) {
            const double w = (double)s_kw[mem];
            double gw = 0.0;
            if (w > 0.0 && kappa > 0.0f)
                gw = (((double)s_coef[mem] * ((double)dco[mem] - Tk)) * Om - w * To) / (w * Om);
            p.d_omega[s_slot[mem]] = (float)gw;
        }
    }
    if (p.variant == PN_VARIANT_HETERO) {
        float tot = 0.0f;
        for (int mem = tid; mem < W; mem += 256) tot += s_coef[mem] * dco[mem];
        tot = wave_sum(tot);
        if (lane == 0) s_tot[wave] = tot;
        __syncthreads();
        tot = ((s_tot[0] + s_tot[1]) + (s_tot[2] + s_tot[3])) * (kappa > 0.0f ? 1.0f / kappa : 0.0f);
        for (int mem = tid; mem < W; mem += 256) {
            const int64_t s = (int64_t)g * W + mem;
            dsc[mem] = s_coef[mem] * (dco[mem] - tot) * (p.rawsc[s] > 0.0f ? 1.0f : 0.01f);
        }
    } else {
        for (int mem = tid; mem < W; mem += 256)
            dsc[mem] = p.variant == PN_VARIANT_HOMO ? (p.omega ? (kappa * s_kw[mem]) * dco[mem] : dco[mem]) : 0.0f;
    }
    __syncthreads();
    // per member: d h_n, the attention-weight terms and the attention-ego term; wave w takes members w, w + 4, ...
    float gaw_h[HI], gaw_e[HI], ego_acc[HI], gab = 0.0f;
#pragma unroll
    for (int i = 0; i < HI; i++) gaw_h[i] = gaw_e[i] = ego_acc[i] = 0.0f;
    const bool has_att = p.variant != PN_VARIANT_PAGG;
    // the members' ego rows: usually one row for the whole group (HOMO: all W paths of a node start at the node) -- then the
    // waves' sums meet in LDS and the group flushes once; otherwise (HETERO, or paths that start elsewhere) a row per
    // member, flushed as it comes
    int same = 1;
    for (int mem = tid; mem < W; mem += 256) same &= s_erow[mem] == s_erow[0];
    const bool one_row = __syncthreads_and(same) != 0;
#pragma unroll 2
    for (int mem = wave; mem < W; mem += 4) {
        const int64_t s = (int64_t)g * W + mem;
        const float ds = dsc[mem], cf = s_coef[mem];
        const int64_t erow = (int64_t)s_erow[mem] * H;
#pragma unroll
        for (int i = 0; i < HI; i++) {
            const int j = lane + 64 * i;
            if (j < H) {
                float dh = cf * dp[j];
                if (has_att) {
                    dh += ds * p.att_w[j];
                    gaw_h[i] += ds * p.hn[s * H + j];
                    gaw_e[i] += ds * p.ego_tab[erow + j];
                    const float eg = ds * p.att_w[H + j];
                    if (one_row)
                        ego_acc[i] += eg;
                    else if (!p.det_ds)
                        atomicAdd(&p.dego[erow + j], eg);
                }
                if (p.g_state) dh += p.g_state[s * H + j];
                p.dhn[s * H + j] = dh;
            }
        }
        gab += ds;
        if (p.det_ds && lane == 0) p.det_ds[s] = ds;
    }
    if (!has_att) return;       // block-uniform
    if (one_row && !p.det_ds) {
#pragma unroll
        for (int i = 0; i < HI; i++) {
            const int j = lane + 64 * i;
            if (j < H) red[wave * H + j] = ego_acc[i];
        }
        __syncthreads();
        const int64_t erow = (int64_t)s_erow[0] * H;
        for (int j = tid; j < H; j += 256)
            atomicAdd(&p.dego[erow + j], (red[j] + red[H + j]) + (red[2 * H + j] + red[3 * H + j]));
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < HI; i++) {
        const int j = lane + 64 * i;
        if (j < H) {
            red[wave * 2 * H + j] = gaw_h[i];
            red[wave * 2 * H + H + j] = gaw_e[i];
        }
    }
    __syncthreads();
    float *out = p.det_att + (int64_t)blockIdx.x * (2 * H + 4);
    for (int j = tid; j < 2 * H; j += 256) out[j] = red[j] + red[2 * H + j] + red[4 * H + j] + red[6 * H + j];
    if (lane == 0) out[2 * H + wave] = gab;
}
template <int HI>
__global__ __launch_bounds__(256) void pool_bwd_wg_kernel(PoolBwdParams p) {
    extern __shared__ float lds[];
    pool_bwd_wg_body<HI>(p, lds);
}
inline size_t pool_bwd_lds_bytes(int W, int H) {
    return (4 * (2 * (size_t)W + (size_t)H) + 8 * (size_t)H + 8 * (size_t)W) * sizeof(float);
}

// ---- pooling forward, loss and pooling backward of a group in ONE launch (PoolStepParams / PoolStepLossParams: pn_pool.h) ----
template <int HI>
__global__ __launch_bounds__(256) void pool_step_kernel(PoolStepParams p) {
    extern __shared__ float lds[];
    pool_fwd_body(p.f, lds);
    __syncthreads();            // (workgroup-scope fence: out[g, :] written above is visible below; LDS is free again)
    if (threadIdx.x == 0) {     // the row's cross entropy exactly as cross_entropy_kernel computes it
        const int g = blockIdx.x, classes = p.f.C;
        const float *x = p.f.out + (int64_t)g * classes;
        float m = x[0];
        for (int c = 1; c < classes; c++) m = fmaxf(m, x[c]);
        float sum = 0.0f;
        for (int c = 0; c < classes; c++) sum += expf(x[c] - m);
        const float ls = logf(sum);
        const int64_t t64 = p.target[g];        // out of range: NaN loss, zero gradient row, no address formed from it
        const bool ok = t64 >= 0 && t64 < (int64_t)classes;
        const int t = ok ? (int)t64 : 0;
        const float row = ls - (x[t] - m);
        p.lossg[g] = ok ? row : NAN;
        float *go = p.gout + (int64_t)g * classes;
        for (int c = 0; c < classes; c++) {
            const float gv = (expf((x[c] - m) - ls) - (c == t ? 1.0f : 0.0f)) * p.scale;
            go[c] = ok ? gv : 0.0f;
        }
    }
    __syncthreads();
    pool_bwd_wg_body<HI>(p.b, lds);
}
template <int HI>
__global__ __launch_bounds__(256) void pool_step_loss_kernel(PoolStepLossParams q) {
    extern __shared__ float lds[];
    const PoolStepParams &p = q.s;
    pool_fwd_body(p.f, lds);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int g = blockIdx.x, classes = p.f.C;
        float k_grad, k_loss;
        loss_factors(q.o, k_grad, k_loss);
        p.lossg[g] = ce_row_opts(p.f.out + (int64_t)g * classes, classes, p.target[g], q.o, k_grad, p.gout + (int64_t)g * classes);
    }
    __syncthreads();
    pool_bwd_wg_body<HI>(p.b, lds);
}
// ---- the same step with the node's rows held in REGISTERS (round 6).  pool_step_kernel's bodies change the thread layout from
// phase to phase (eight lanes per member for the dot products, a lane per column for the sums) and therefore read the node's
// W x H final hidden states four times from memory, behind one another: ~15 dependent round trips per node, 47 us for 1 299
// nodes and 0.27 / 1.3 ms at Pubmed / BGP size, where the launch is bound by that cache traffic.  Here wave w owns members
// w, w + 4, ... (MM of them) and a lane columns lane + 64 i (HI of them) throughout: the rows are loaded ONCE, all at once
// (MM x HI registers), dot products over H are wave sums, sums over W are lane-local plus one exchange through LDS -- five
// round trips and eight barriers per node.  Same arithmetic, other summation orders than the three kernels (which the
// deterministic mode keeps: pn_pagg_train_step's bitwise tests run there); W <= 4 MM, H <= 64 HI.
#ifdef PN_POOL_TRACE
__device__ long long g_pool_trace[2048 * 12];
#define PTRACE(n) do { if (threadIdx.x == 0 && blockIdx.x < 2048) g_pool_trace[blockIdx.x * 12 + (n)] = wall_clock64(); } while (0)
#else
#define PTRACE(n) do { } while (0)
#endif
// (the kernel's text: pn_pool_step2.inc, once as pool_step2_kernel, once with the loss options as pool_step2_loss_kernel)
#include "pn_pool_step2.inc"
#define PN_STEP2_LOSS_OPTS
#include "pn_pool_step2.inc"
#undef PN_STEP2_LOSS_OPTS
inline size_t pool_step2_lds_bytes(int MM, int H, int C) { return (size_t)(12 * MM + 8 * H + 2 * H + H + 2 * C + 8) * sizeof(float); }

// loss[0] (+)= scale * sum of the rows' terms, in cross_entropy_kernel's order (one workgroup of 1024 threads)
__global__ __launch_bounds__(1024) void loss_sum_kernel(const float *__restrict__ lossg, int rows, float scale,
                                                        float *__restrict__ loss, int store) {
    __shared__ float part[16];
    float mine = 0.0f;
    for (int r = threadIdx.x; r < rows; r += 1024) mine += lossg[r];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.0f;
        for (int w = 0; w < 16; w++) t += part[w];
        if (store)
            *loss = t * scale;
        else
            atomicAdd(loss, t * scale);
    }
}

// the same with the options' k = grad_scale / D (mean) or grad_scale (sum), formed here from D in device memory
__global__ __launch_bounds__(1024) void loss_sum_opts_kernel(const float *__restrict__ lossg, int rows, LossOpts o,
                                                             float *__restrict__ loss, int store) {
    __shared__ float part[16];
    float mine = 0.0f;
    for (int r = threadIdx.x; r < rows; r += 1024) mine += lossg[r];
#pragma unroll
    for (int of = 32; of > 0; of >>= 1) mine += __shfl_xor(mine, of, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        float k_grad, k_loss;
        loss_factors(o, k_grad, k_loss);
        float t = 0.0f;
        for (int w = 0; w < 16; w++) t += part[w];
        if (store)
            *loss = t * k_loss;
        else
            atomicAdd(loss, t * k_loss);
    }
}

// the pooling backward's per-workgroup attention terms ([nblk][2H + 4]: g_att_w partials, then one g_att_b term per
// wave) added up in a fixed order.  A workgroup owns 64 consecutive outputs: sixteen row groups of 64 lanes walk the
// partials' rows 16 apart -- every load a 256-byte run of one row -- and meet in LDS (round 6; a workgroup per output read
// the [nblk][260] array column-wise, one cache line per element: 19 us for 1.3 MB at the headline shape)
__global__ __launch_bounds__(1024) void det_att_reduce_kernel(const float *__restrict__ part, int nblk, int H,
                                                              float *__restrict__ g_att_w, float *__restrict__ g_att_b) {
    __shared__ float red[16][64];
    const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6, stride = 2 * H + 4;
    const int col = blockIdx.x * 64 + lane;
    float v = 0.0f;
    if (col < stride) {
        const float *src = part + col;
#pragma unroll 8
        for (int b = rg; b < nblk; b += 16) v += src[(int64_t)b * stride];
    }
    red[rg][lane] = v;
    __syncthreads();
    if (rg != 0) return;
    float t = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; r++) t += red[r][lane];
    if (col < 2 * H) {
        g_att_w[col] += t;
    } else if (col < stride) {      // the four per-wave bias terms sit in one workgroup (4 | 2H): lanes c .. c + 3
        red[0][lane] = t;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (col == 2 * H) *g_att_b += (red[0][lane] + red[0][lane + 1]) + (red[0][lane + 2] + red[0][lane + 3]);
    }
}

}  // namespace

namespace pn {

// (also what pool_step_kernel allocates: its three bodies share one carving)
size_t pool_lds_bytes(int W, int H) { return std::max(pool_bwd_lds_bytes(W, H), pool_fwd_lds_bytes(W, H)); }

int launch_pool_fwd(void *stream, const PoolParams &p) {
    hipLaunchKernelGGL(pool_fwd_kernel, dim3(p.S), dim3(256), pool_fwd_lds_bytes(p.W, p.H), (hipStream_t)stream, p);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int launch_pool_bwd(pn_context *ctx, void *stream, const PoolBwdParams &p) {
    const size_t lds_bytes = pool_bwd_lds_bytes(p.W, p.H);
    if (p.H <= 256) {
        hipLaunchKernelGGL(pool_bwd_wg_kernel<4>, dim3(p.S), dim3(256), lds_bytes, (hipStream_t)stream, p);
    } else {
        if (int rc = ensure_dynamic_lds(ctx, reinterpret_cast<const void *>(pool_bwd_wg_kernel<16>), (int)lds_bytes)) return rc;
        hipLaunchKernelGGL(pool_bwd_wg_kernel<16>, dim3(p.S), dim3(256), lds_bytes, (hipStream_t)stream, p);
    }
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int launch_pool_step(pn_context *ctx, void *stream, const PoolStepParams &ps, const LossOpts *opts, int knob) {
    hipStream_t s = (hipStream_t)stream;
    const int W = ps.f.W, H = ps.f.H, C = ps.f.C, Sb = ps.f.S;
    const size_t lds_step = pool_lds_bytes(W, H);
    // pool_step2_kernel holds the logits and their gradient in LDS (2 C floats; 6 144 + 8 C bytes at H = 128), which
    // pool_lds_bytes does not bound: past 64 KiB (C > 7 424 at H = 128) the node goes to pool_step_kernel<4>, whose LDS does
    // not depend on C (within 64 KiB by make_dims)
    const size_t lds_step2 = pool_step2_lds_bytes(10, H, C);
    // (pool_step2_kernel does not carry the path weights: a weighted call takes the three bodies)
    const bool step2 = W <= 40 && H <= 128 && H >= 32 && lds_step2 <= 64 * 1024 && knob >= 1 && knob != 2 && !ps.f.omega;
    if (opts) {         // pn_pagg_train_step_loss: the same three routes, their option-aware kernels
        const PoolStepLossParams ql{ps, *opts};
        if (step2) {
            hipLaunchKernelGGL((pool_step2_loss_kernel<10, 2>), dim3(Sb), dim3(256), lds_step2, s, ql);
        } else if (H <= 256) {
            hipLaunchKernelGGL(pool_step_loss_kernel<4>, dim3(Sb), dim3(256), lds_step, s, ql);
        } else {
            if (int rc = ensure_dynamic_lds(ctx, reinterpret_cast<const void *>(pool_step_loss_kernel<16>), (int)lds_step)) return rc;
            hipLaunchKernelGGL(pool_step_loss_kernel<16>, dim3(Sb), dim3(256), lds_step, s, ql);
        }
    } else if (step2) {
        // the node's rows in registers (pool_step2_kernel); PN_POOL_STEP=2: the three bodies back to back
        hipLaunchKernelGGL((pool_step2_kernel<10, 2>), dim3(Sb), dim3(256), lds_step2, s, ps);
    } else if (H <= 256) {
        hipLaunchKernelGGL(pool_step_kernel<4>, dim3(Sb), dim3(256), lds_step, s, ps);
    } else {
        if (int rc = ensure_dynamic_lds(ctx, reinterpret_cast<const void *>(pool_step_kernel<16>), (int)lds_step)) return rc;
        hipLaunchKernelGGL(pool_step_kernel<16>, dim3(Sb), dim3(256), lds_step, s, ps);
    }
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int launch_loss_sum(void *stream, const float *lossg, int rows, float scale, const LossOpts *opts, float *loss, bool store) {
    if (opts)
        hipLaunchKernelGGL(loss_sum_opts_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, lossg, rows, *opts, loss, store ? 1 : 0);
    else
        hipLaunchKernelGGL(loss_sum_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, lossg, rows, scale, loss, store ? 1 : 0);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int launch_att_reduce(void *stream, const float *part, int nblk, int H, float *g_att_w, float *g_att_b) {
    hipLaunchKernelGGL(det_att_reduce_kernel, dim3((2 * H + 4 + 63) / 64), dim3(1024), 0, (hipStream_t)stream, part, nblk, H, g_att_w,
                       g_att_b);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

}  // namespace pn

#ifdef PN_POOL_TRACE
extern "C" int pn_debug_pool_trace(long long *host_out) {
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_pool_trace), sizeof(long long) * 2048 * 12) == hipSuccess ? 0 : -1;
}
#endif
