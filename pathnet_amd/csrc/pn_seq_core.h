// pn_seq_core.h -- what the recurrent kernels of pn_seqh.hip (fp16 x 2 planes), pn_seq3.hip (bf16 x 3 planes) and pn_seqgen.hip
// (step by step, above H = 256) have in common, written once: the cell functions and their derivatives, the source half of
// the weight packings, the dropout pieces of the gather and the scatter, the description of a kernel's tile with its LDS
// layout, and the launch glue (hidden-size dispatch, launch helper).  What differs between the arithmetics -- scaling,
// splitting into planes, the saved-tensor layouts, the MFMA loops -- stays in the kernels.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pn_internal.h"
#include "pn_kernels.h"
#include "pn_seq.h"

namespace pn {

// ================================================================================================
// The cells.  Forward: pre-activations (bias included, operand scales divided out) and the previous state in, gates, new
// state and h out.  Backward: the forward's saved values, dh (and the carried dc) in, the gradients of the four gate slots'
// pre-activations and the value carried to step t - 1 out; `ok` is false for the padded rows of a ragged tile, whose
// gradients are zero.  The expressions are the ones every kernel had: the compiler contracts them to the same FMAs.
// ================================================================================================
struct LstmFwd {
    float ig, fg, gg, og, c, h;
};
__device__ __forceinline__ LstmFwd lstm_fwd(float pi, float pf, float pg, float po, float cprev) {
    LstmFwd o;
    o.ig = sigmoidf_(pi);
    o.fg = sigmoidf_(pf);
    o.gg = tanhf_(pg);
    o.og = sigmoidf_(po);
    o.c = o.fg * cprev + o.ig * o.gg;
    o.h = o.og * tanhf_(o.c);
    return o;
}
// GRU on the LSTM's four gate slots (torch gate order r, z, n; n = tanh(W_in x + b_in + r * (W_hn h + b_hn))): slot 0 = r and
// 1 = z over [x | h] as usual, slot 2 = "nx" = W_in x + b_in (its h half of the weights is zero), slot 3 = "nh" = W_hn h + b_hn
// (its x half is zero).  A quarter of the products multiplies zeros; in return the recurrence, its BPTT and the
// weight-gradient GEMM are the LSTM's kernels with another cell function.  Saved: r, z, n, nh, h_{t-1}.
struct GruFwd {
    float rg, zg, ng, nh, h;
};
__device__ __forceinline__ GruFwd gru_fwd(float pr, float pz, float pnx, float pnh, float hp) {
    GruFwd o;
    o.rg = sigmoidf_(pr);
    o.zg = sigmoidf_(pz);
    o.nh = pnh;
    o.ng = tanhf_(pnx + o.rg * o.nh);
    o.h = (1.0f - o.zg) * o.ng + o.zg * hp;
    return o;
}
__device__ __forceinline__ float rnn_fwd(float pre) { return tanhf_(pre); }

struct CellGrad {
    float a0, a1, a2, a3;   // gate slots i, f, g, o (LSTM) / r, z, nx, nh (GRU)
    float carry;    // LSTM: dc of step t - 1;  GRU: the direct path d h_t / d h_{t-1} = z, added to the GEMM's dh output
};
// c = c_t, cprev = c_{t-1} (0 at t = 0), dc = d loss / d c_t from step t + 1
__device__ __forceinline__ CellGrad lstm_bwd(float ig, float fg, float gg, float og, float cprev, float c, float dhv, float dc,
                                             bool ok) {
    const float tc = tanhf_(c);
    const float d_o = dhv * tc;
    const float dct = dc + dhv * og * (1.0f - tc * tc);
    CellGrad o;
    o.a0 = dct * gg * ig * (1.0f - ig);
    o.a1 = dct * cprev * fg * (1.0f - fg);
    o.a2 = dct * ig * (1.0f - gg * gg);
    o.a3 = d_o * og * (1.0f - og);
    if (!ok) o.a0 = o.a1 = o.a2 = o.a3 = 0.0f;
    o.carry = dct * fg;
    return o;
}
// h = (1 - z) n + z h_prev,  n = tanh(nx + r nh)
__device__ __forceinline__ CellGrad gru_bwd(float rg, float zg, float ng, float nh, float hp, float dhv, bool ok) {
    const float dnp = dhv * (1.0f - zg) * (1.0f - ng * ng);
    CellGrad o;
    o.a0 = dnp * nh * rg * (1.0f - rg);
    o.a1 = dhv * (hp - ng) * zg * (1.0f - zg);
    o.a2 = dnp;
    o.a3 = dnp * rg;
    if (!ok) o.a0 = o.a1 = o.a2 = o.a3 = 0.0f;
    o.carry = ok ? dhv * zg : 0.0f;
    return o;
}
__device__ __forceinline__ float rnn_bwd(float h, float dhv, bool ok) { return ok ? dhv * (1.0f - h * h) : 0.0f; }

// ================================================================================================
// Weight packing: where a fragment's values come from.  The kernels scale, split into planes and store.
// ================================================================================================
// bias of element idx of the G*H gate-slot rows: b_ih + b_hh; GRU: slots r, z summed, nx = b_in, nh = b_hn
__device__ __forceinline__ float packed_bias(const float *__restrict__ b_ih, const float *__restrict__ b_hh, int64_t idx, int H,
                                             int gru) {
    if (!gru) return b_ih[idx] + b_hh[idx];
    const int slot = (int)(idx / H), j = (int)(idx - (int64_t)slot * H), wr = gru_weight_row(slot, j, H);
    return slot < 2 ? b_ih[wr] + b_hh[wr] : slot == 2 ? b_ih[wr] : b_hh[wr];
}

// forward B fragment idx < pack_fwd_count (16 bytes per plane):  Wcat[g*H + 32w + (lane & 31)][16 s + 8 (lane >> 5) .. +7],
// stored at Wp[((unit * PLANES + plane) * G + g) * 64 + lane] with unit = w * KS + s, KS = 2H/16 k-steps
struct PackFwdSrc {
    float4 v0, v1;
    int unit, g, lane;
    bool xhalf;         // the eight values are W_ih's (else W_hh's)
};
__device__ __forceinline__ int pack_fwd_count(int H, int G) { return (H / 32) * (H / 8) * G * 64; }
__device__ __forceinline__ PackFwdSrc pack_fwd_src(int idx, const float *__restrict__ w_ih, const float *__restrict__ w_hh, int H,
                                                   int G, int gru) {
    const int KS = H / 8;
    const int lane = idx & 63;
    int rest = idx >> 6;
    const int g = rest % G;
    rest /= G;
    const int s = rest % KS, w = rest / KS;
    const int j = 32 * w + (lane & 31), k = 16 * s + 8 * (lane >> 5);
    const int row = gru ? gru_weight_row(g, j, H) : g * H + j;
    const float *src = k < H ? w_ih + (int64_t)row * H + k : w_hh + (int64_t)row * H + (k - H);
    float4 v0 = reinterpret_cast<const float4 *>(src)[0], v1 = reinterpret_cast<const float4 *>(src)[1];
    if (gru && ((g == 2 && k >= H) || (g == 3 && k < H))) v0 = v1 = make_float4(0.f, 0.f, 0.f, 0.f);
    return PackFwdSrc{v0, v1, w * KS + s, g, lane, k < H};
}
// BPTT B fragment: the eight values Wcat[k .. k+7][nt*H + n] (nt == 0: the dx half, W_ih).  The index decode stays with
// the packing kernels (profiles/seq_core.txt).
__device__ __forceinline__ void pack_bwd_src(int k, int n, int nt, const float *__restrict__ w_ih, const float *__restrict__ w_hh, int H,
                                             int gru, float (&v)[8]) {
    if (!gru) {
        const float *src = (nt == 0 ? w_ih : w_hh) + (int64_t)k * H + n;
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] = src[(int64_t)e * H];
    } else {        // k .. k+7 lie inside one gate slot (8 | H)
        const int slot = k / H, j = k - slot * H;
        const bool zero = (slot == 2 && nt == 1) || (slot == 3 && nt == 0);
        const float *src = (nt == 0 ? w_ih : w_hh) + (int64_t)gru_weight_row(slot, j, H) * H + n;
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] = zero ? 0.0f : src[(int64_t)e * H];
    }
}

// ================================================================================================
// Dropout pieces of the forward's gather and the BPTT's scatter.  (Applying a keep nibble or an explicit-mask float4 to a
// gathered row stays written out in the two forward kernels: profiles/seq_core.txt.)
// ================================================================================================
// which of a dropout4 draw's four elements are kept, bits 0-3 (the layout of SeqFwdParams::keep)
__device__ __forceinline__ uint32_t keep_nibble(const float4 &m) {
    return (m.x != 0.f ? 1u : 0u) | (m.y != 0.f ? 2u : 0u) | (m.z != 0.f ? 4u : 0u) | (m.w != 0.f ? 8u : 0u);
}
// dx of column col under the keep byte of columns col & ~3 .. + 3
__device__ __forceinline__ float keep_dx(float dx, uint32_t keep_byte, int col, float keep_scale) {
    return (keep_byte >> (col & 3)) & 1 ? dx * keep_scale : 0.0f;
}

// ================================================================================================
// The tile of one workgroup: MT = 32 paths, wave w owns hidden units 32w .. 32w+31 of all gate slots.  GC: 4 = LSTM,
// 1 = tanh RNN, 3 = GRU on the LSTM's four gate slots; PLANES: 2 (fp16) or 3 (bf16).  The kernels take their LDS pointers and
// the launchers their dynamic LDS size from here: each layout is written down once, pointers and size side by side.
// ================================================================================================
template <int H_, int GC_, int PLANES_>
struct SeqTile {
    static constexpr int H = H_, GC = GC_, PLANES = PLANES_;
    static constexpr int G = GC == 3 ? 4 : GC;
    static constexpr bool GRU = GC == 3;
    static constexpr int MT = 32, NW = H / 32, NT = NW * 64, GH = G * H;
    static constexpr int SV = G == 4 ? 5 : 1;           // saved values per (path step, unit) in [SV][H] planes
    // forward: PLANES planes of [MT][x_t | h_{t-1}], 2 bytes an element, row pitch + 16: conflict-free ds_read_b128
    //          | rowidx [MT][L] | slotof [MT]
    static constexpr int FWD_PB = 4 * H + 16, FWD_PLANE = MT * FWD_PB;
    static __device__ __forceinline__ int *fwd_rowidx(unsigned char *lds) { return reinterpret_cast<int *>(lds + PLANES * FWD_PLANE); }
    static __device__ __forceinline__ int *fwd_slotof(unsigned char *lds, int L) { return fwd_rowidx(lds) + MT * L; }
    static constexpr int fwd_lds_bytes(int L) { return PLANES * FWD_PLANE + (MT * L + MT) * 4; }
    // pre-projected forward: the tile holds h_{t-1} only | rowidx [MT][L]
    static constexpr int ZW_PB = 2 * H + 16, ZW_PLANE = MT * ZW_PB;
    static __device__ __forceinline__ int *zw_rowidx(unsigned char *lds) { return reinterpret_cast<int *>(lds + PLANES * ZW_PLANE); }
    static constexpr int zw_lds_bytes(int L) { return PLANES * ZW_PLANE + MT * L * 4; }
    // BPTT: planes of dG_t [MT][KP].  Two planes hold all four gates; three would take 96 KB at H = 128, so the bf16 tile
    //       holds one gate pair at a time (NPASS = 2 passes of the k loop)
    //       | rowidx [MT * L] | slotof [MT] | fp16: wave maxima of |dG_t| [8] | keep bits of step t, in half t & 1 [2][MT][H/4]
    static constexpr int NPASS = PLANES == 3 && G == 4 ? 2 : 1, KP = GH / NPASS;
    static constexpr int BWD_PB = 2 * KP + 16, BWD_PLANE = MT * BWD_PB, SMAX = PLANES == 2 ? 8 : 0;
    static __device__ __forceinline__ int *bwd_rowidx(unsigned char *lds) { return reinterpret_cast<int *>(lds + PLANES * BWD_PLANE); }
    static __device__ __forceinline__ int *bwd_slotof(unsigned char *lds, int L) { return bwd_rowidx(lds) + MT * L; }
    static __device__ __forceinline__ float *bwd_smax(unsigned char *lds, int L) { return reinterpret_cast<float *>(bwd_slotof(lds, L) + MT); }
    static __device__ __forceinline__ uint8_t *bwd_keep(unsigned char *lds, int L) { return reinterpret_cast<uint8_t *>(bwd_smax(lds, L) + SMAX); }
    static constexpr int bwd_lds_bytes(int L) { return PLANES * BWD_PLANE + (MT * L + MT) * 4 + SMAX * 4 + 2 * MT * (H / 4); }
};

// ================================================================================================
// Launch glue (host)
// ================================================================================================
// f(integral_constant<int, H>, integral_constant<int, GC>) for the hidden sizes the fused kernels are built for: every
// multiple of 32 up to 256 (the BPTT's LDS tile of H = 256 is 98 KB in bf16, 133 KB in fp16)
template <class F>
int dispatch_seq(int H, int gc, F &&f) {
    auto by_h = [&](auto gcc) {
        switch (H) {
            case 32: return f(std::integral_constant<int, 32>{}, gcc);
            case 64: return f(std::integral_constant<int, 64>{}, gcc);
            case 96: return f(std::integral_constant<int, 96>{}, gcc);
            case 128: return f(std::integral_constant<int, 128>{}, gcc);
            case 160: return f(std::integral_constant<int, 160>{}, gcc);
            case 192: return f(std::integral_constant<int, 192>{}, gcc);
            case 224: return f(std::integral_constant<int, 224>{}, gcc);
            case 256: return f(std::integral_constant<int, 256>{}, gcc);
        }
        PN_FAIL(PN_ERR_ARG, "hidden size %d not supported", H);
    };
    return gc == 3 ? by_h(std::integral_constant<int, 3>{}) : gc == 4 ? by_h(std::integral_constant<int, 4>{})
                                                                     : by_h(std::integral_constant<int, 1>{});
}

// a kernel with dynamic LDS: the size is registered with the context once, then launch + error check
template <class... KArgs, class... Args>
int launch_with_lds(pn_context *ctx, void *stream, void (*kern)(KArgs...), dim3 grid, dim3 block, int lds_bytes, const Args &...args) {
    if (int rc = ensure_dynamic_lds(ctx, reinterpret_cast<const void *>(kern), lds_bytes)) return rc;
    hipLaunchKernelGGL(kern, grid, block, (size_t)lds_bytes, (hipStream_t)stream, args...);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}
// one of the recurrent kernels over the tiles of `paths` paths
template <class T, class Params>
int launch_seq_tiles(pn_context *ctx, void *stream, void (*kern)(Params), int lds_bytes, const Params &sp) {
    return launch_with_lds(ctx, stream, kern, dim3((sp.P + T::MT - 1) / T::MT), dim3(T::NT), lds_bytes, sp);
}

}  // namespace pn
