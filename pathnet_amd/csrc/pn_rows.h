// pn_rows.h -- what the builders that start from edge rows share (pn_tables.hip: the sampler's tables; pn_census.hip: the
// multiset neighbour lists): the workspace carver, the range check of the rows with its one-word read-back, and the
// bucket offsets of a sorted key array.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pathnet_hip.h"
#include "pn_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 65536;

int blocks_for(int64_t items) {
    int64_t b = (items + kThreads - 1) / kThreads;
    return b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : (int)b);
}

int key_bits_for(int32_t n) {
    int bits = 1;
    while (bits < 31 && (1LL << bits) < (int64_t)n) bits++;
    return bits;
}

// bump allocator over the caller's workspace (base == nullptr: sizing only)
struct Carver {
    char *base;
    size_t at = 0;
    template <class T>
    T *take(size_t count) {
        at = (at + 255) & ~(size_t)255;
        T *p = base ? reinterpret_cast<T *>(base + at) : nullptr;
        at += count * sizeof(T);
        return p;
    }
};

// *status = min(e) over the rows with a source or a target outside [0, n)
__global__ __launch_bounds__(kThreads) void validate_kernel(int32_t n, int64_t m, const int32_t *__restrict__ u,
                                                            const int32_t *__restrict__ v,
                                                            unsigned long long *__restrict__ status) {
    for (int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x; e < m; e += (int64_t)gridDim.x * kThreads) {
        const int32_t a = u[e], b = v[e];
        if (a < 0 || a >= n || b < 0 || b >= n) atomicMin(status, (unsigned long long)e);
    }
}

// first index of the sorted keys[0, m) holding a key >= x
__device__ int64_t lower_bound(const int32_t *__restrict__ keys, int64_t m, int32_t x) {
    int64_t lo = 0, hi = m;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// off[x] = first bucketed row of node x, x in [0, n]
__global__ __launch_bounds__(kThreads) void bucket_off_kernel(int32_t n, int64_t m, const int32_t *__restrict__ keys,
                                                              int64_t *__restrict__ off) {
    for (int64_t x = blockIdx.x * (int64_t)kThreads + threadIdx.x; x <= n; x += (int64_t)gridDim.x * kThreads)
        off[x] = lower_bound(keys, m, (int32_t)x);
}

// launch validate_kernel and return the first out-of-range row (or -1); synchronises with the stream
int first_bad_row(int32_t n, int64_t m, const int32_t *u, const int32_t *v, unsigned long long *status,
                  hipStream_t stream, int64_t *row) {
    unsigned long long h = ~0ull;
    PN_CHECK_HIP(hipMemsetAsync(status, 0xff, sizeof h, stream));
    if (m > 0) hipLaunchKernelGGL(validate_kernel, dim3(blocks_for(m)), dim3(kThreads), 0, stream, n, m, u, v, status);
    PN_CHECK_HIP(hipGetLastError());
    PN_CHECK_HIP(hipMemcpyAsync(&h, status, sizeof h, hipMemcpyDeviceToHost, stream));
    PN_CHECK_HIP(hipStreamSynchronize(stream));
    *row = h == ~0ull ? -1 : (int64_t)h;
    return PN_OK;
}

int read_row(const int32_t *u, const int32_t *v, int64_t e, int32_t *a, int32_t *b, hipStream_t stream) {
    PN_CHECK_HIP(hipMemcpyAsync(a, u + e, sizeof *a, hipMemcpyDeviceToHost, stream));
    PN_CHECK_HIP(hipMemcpyAsync(b, v + e, sizeof *b, hipMemcpyDeviceToHost, stream));
    PN_CHECK_HIP(hipStreamSynchronize(stream));
    return PN_OK;
}

}  // namespace
