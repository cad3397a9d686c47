// pn_group.h -- the thread groups that own one row of C classes, shared by pn_ensemble.hip and pn_calib.hip.
//
// Work split: G depends on C alone.
//   C <= 16           G = 1    a thread per row: the class loop is the ascending serial sum
//   16 < C <= 1024    G = 64   a wave per row, four rows per workgroup: lane l holds classes l, l + 64, ...
//   1024 < C <= 4096  G = 256  a workgroup per row
// Order of a sum over classes: every lane adds its own classes in ascending c, the 64 lane sums meet in a butterfly
// (xor 32, 16, ..., 1: fp addition commutes, so every lane holds the same bits), the four wave sums of a workgroup are added
// as (w0 + w1) + (w2 + w3).  That order is a function of C and nothing else, and for G = 1 it is the plain ascending sum.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pn {
namespace group {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1 << 16;          // rows beyond that are taken in a grid-stride loop
constexpr int kThreadMaxC = 16;              // C <= 16: a thread per row
constexpr int kWaveMaxC = 1024;              // C <= 1024: a wave per row
constexpr int kMaxC = 4096;

inline int group_of(int32_t C) { return C <= kThreadMaxC ? 1 : C <= kWaveMaxC ? 64 : 256; }

inline unsigned blocks_for(int64_t n, int G) {
    const int64_t per_block = kThreads / G;
    const int64_t need = (n + per_block - 1) / per_block;
    return (unsigned)(need < kMaxBlocks ? need : kMaxBlocks);
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

// false for NaN and both infinities
__device__ inline bool finite_f32(float v) { return fabsf(v) <= 3.4028234663852886e38f; }

}  // namespace group
}  // namespace pn
