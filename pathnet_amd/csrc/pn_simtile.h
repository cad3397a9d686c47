// pn_simtile.h -- the exact-fp32 similarity tile that pn_contrast.hip and pn_knn.hip share: a workgroup of 256 computes
// <z_row, z_col> for a 64 x 128 tile of row / column pairs of ONE stacked array Z [n, D], over K chunks of 16 on
// v_mfma_f32_32x32x2_f32 -- exact fp32 products, one k-ordered fma chain per element, so <z_r, z_c> and <z_c, z_r> have the same
// bits wherever the pair is computed.  Every translation unit that includes this gets its own copy (anonymous namespace).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 256;
constexpr int kRT = 64;                  // row tile: 2 x 32 rows (wave w: rows 32 (w >> 1) ..)
constexpr int kCT = 128;                 // column tile: 2 x 64 columns (wave w: columns 64 (w & 1) ..)
constexpr int kKC = 16;                  // K chunk staged in LDS

static_assert(kKC % 2 == 0 && kCT % 2 == 0, "the MFMA takes two k per issue");

// ---- the logits of one (row tile, column tile) -----------------------------------------------------------------------------------
struct Stage {
    float a[kKC][kRT + 1];
    float b[kKC][kCT + 1];
};

// acc[j][i] = <z_row, z_col>, row = r0 + 32 (w >> 1) + 8 (i >> 2) + 4 (lane >> 5) + (i & 3), col = c0 + 64 (w & 1) + 32 j +
// (lane & 31).  Rows / columns past n and k past D enter as zeros: an exact + 0 at the end of the chain.
__device__ inline void logits_tile(const float *__restrict__ Z, int64_t n, int32_t D, int64_t r0, int64_t c0, Stage &st,
                                   f32x16 acc[2]) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int arow = 32 * (wv >> 1) + (lane & 31), bcol = 64 * (wv & 1) + (lane & 31), kh = lane >> 5;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[0][i] = acc[1][i] = 0.0f;
    for (int32_t k0 = 0; k0 < D; k0 += kKC) {
        __syncthreads();
        for (int e = t; e < kRT * kKC; e += kThreads) {
            const int row = e / kKC, kk = e % kKC;
            const int64_t r = r0 + row;
            st.a[kk][row] = (r < n && k0 + kk < D) ? Z[r * D + k0 + kk] : 0.0f;
        }
        for (int e = t; e < kCT * kKC; e += kThreads) {
            const int col = e / kKC, kk = e % kKC;
            const int64_t c = c0 + col;
            st.b[kk][col] = (c < n && k0 + kk < D) ? Z[c * D + k0 + kk] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kKC; kk += 2) {
            const float a = st.a[kk + kh][arow];
            const float b0 = st.b[kk + kh][bcol];
            const float b1 = st.b[kk + kh][bcol + 32];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc[1], 0, 0, 0);
        }
    }
}

}  // namespace
