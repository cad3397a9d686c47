// pn_det.hip -- the deterministic scatter-add of the aggregator's backward on gfx950.  Launch parameters and launchers: pn_det.h.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pn_det.h"
#include "pn_internal.h"

using namespace pn;

namespace {

// ================================================================================================
// Deterministic scatter-add (pn_pagg_shape.deterministic): dst[key[i]] += contribution i, added in the order of i.
// The default backward scatters with fp32 atomics, whose order -- and with it the last bits of every gradient -- changes
// from run to run (the reference inherits the same from torch's index_add / embedding backward).
// Here the (key, i) pairs are sorted by key (stable radix sort, pn_sort.hip), the sorted array is cut into chunks of
// DET_CHUNK positions, and one group of H/4 lanes walks a chunk in order:
//   pass 1  a run of equal keys that lies inside the chunk is added to dst by its one owner; a run that crosses a chunk
//           boundary leaves its piece in cpart[chunk][lead | trail];
//   pass 2  the chunk holding the head of a crossing run adds the pieces up in chunk order and adds the sum to dst.
// Every dst row has exactly one writer per pass and a fixed order of additions: bitwise reproducible.
// A contribution is a row of `rows` ([K, H]) or scal[i] * vec[0..H) (the attention-ego term of the pooling backward).
// The BPTT kernels need no second version for this: in deterministic mode they are handed the identity as their row
// index and the zero-filled contribution buffer as their table -- every atomic then lands on an address of its own,
// i.e. is a store -- and the scatter proper happens here.
// ================================================================================================
// (DET_CHUNK, DetScatterParams, DetScatterPair: pn_det.h)
template <int PASS>
__global__ __launch_bounds__(256) void det_scatter_kernel(DetScatterPair pp) {
    const DetScatterParams &p = pp.s[blockIdx.y];
    const int hv = p.H / 4, gpb = 256 / hv;
    const int grp = threadIdx.x / hv, ln = threadIdx.x - grp * hv;
    if (grp >= gpb) return;
    const int64_t c = (int64_t)blockIdx.x * gpb + grp, b = c * DET_CHUNK;
    if (b >= p.K) return;
    const int64_t e = min(p.K, b + (int64_t)DET_CHUNK);
    float4 *dst = reinterpret_cast<float4 *>(p.dst);
    float4 *cpart = reinterpret_cast<float4 *>(p.cpart) + p.chunk0 * 2 * hv;
    const int32_t km = p.kmask;
    auto add_to = [&](float4 *d, const float4 &a) {
        float4 v = *d;
        v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
        *d = v;
    };
    if (PASS == 1) {
        const float4 vec = p.rows ? make_float4(0.f, 0.f, 0.f, 0.f) : reinterpret_cast<const float4 *>(p.vec)[ln];
        int key = p.skey[b] & km;
        bool lead = b > 0 && (p.skey[b - 1] & km) == key;      // the chunk opens inside a run
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        // four positions per trip: their contributions are requested together (the walk was one dependent 512-byte row load
        // per position -- latency, 85 us for the 208 k rows of the headline shape) and added in the order of the positions
        constexpr int DU = 4;
        for (int64_t i0 = b; i0 < e; i0 += DU) {
            int kk[DU];
            float4 vv[DU];
#pragma unroll
            for (int j = 0; j < DU; j++) {
                const int64_t i = min(i0 + j, e - 1);   // (past the end: a harmless re-load of the last position)
                kk[j] = p.skey[i] & km;
                const int64_t src = p.ssrc[i];
                if (p.rows) {
                    vv[j] = reinterpret_cast<const float4 *>(p.rows)[src * hv + ln];
                } else {
                    const float sc = p.scal[src];
                    vv[j] = make_float4(sc * vec.x, sc * vec.y, sc * vec.z, sc * vec.w);
                }
            }
#pragma unroll
            for (int j = 0; j < DU; j++) {
                if (i0 + j >= e) break;
                const int k = kk[j];
                if (k != key) {                          // the run of `key` ends inside the chunk
                    if (lead)
                        cpart[(c * 2 + 0) * hv + ln] = acc;
                    else
                        add_to(dst + (int64_t)key * hv + ln, acc);
                    lead = false;
                    key = k;
                    acc = make_float4(0.f, 0.f, 0.f, 0.f);
                }
                acc.x += vv[j].x; acc.y += vv[j].y; acc.z += vv[j].z; acc.w += vv[j].w;
            }
        }
        const bool cont = e < p.K && (p.skey[e] & km) == key;   // the last run goes on in the next chunk
        if (lead)
            cpart[(c * 2 + 0) * hv + ln] = acc;
        else if (cont)
            cpart[(c * 2 + 1) * hv + ln] = acc;
        else
            add_to(dst + (int64_t)key * hv + ln, acc);
    } else {
        const int key = p.skey[e - 1] & km;
        if (!(e < p.K && (p.skey[e] & km) == key)) return;                      // nothing crosses this chunk's end
        if ((p.skey[b] & km) == key && b > 0 && (p.skey[b - 1] & km) == key) return;   // a middle chunk of the run: its head's chunk adds
        float4 acc = cpart[(c * 2 + 1) * hv + ln];
        for (int64_t c2 = c + 1;; c2++) {
            const int64_t e2 = min(p.K, (c2 + 1) * (int64_t)DET_CHUNK);
            const float4 v = cpart[(c2 * 2 + 0) * hv + ln];
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
            if ((p.skey[e2 - 1] & km) != key || !(e2 < p.K && (p.skey[e2] & km) == key)) break;
        }
        add_to(dst + (int64_t)key * hv + ln, acc);
    }
}

// keys of a scatter, clamped to [0, hi], beside the identity permutation the sort carries along (DetKeys3: pn_det.h)
__global__ __launch_bounds__(256) void det_keys3_kernel(DetKeys3 q, int32_t *__restrict__ keys, int32_t *__restrict__ pos) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t at = i;
    int seg = 0;
    while (seg < 3 && i >= q.n[seg]) i -= q.n[seg], seg++;
    if (seg >= 3) return;
    keys[at] = min(max(q.keys[seg][i], 0), q.hi[seg]) | (seg << q.shift);
    pos[at] = (int32_t)i;
}

__global__ __launch_bounds__(256) void det_iota_kernel(int32_t *__restrict__ iota, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) iota[i] = (int32_t)i;
}

}  // namespace

namespace pn {

int launch_det_scatters(void *stream, const DetScatterParams *list, int count) {
    DetScatterPair pp{};
    int64_t kmax = 0;
    for (int i = 0; i < count; i++) pp.s[i] = list[i], kmax = std::max(kmax, list[i].K);
    if (kmax <= 0) return PN_OK;
    const int gpb = 256 / (list[0].H / 4);          // chunks per workgroup: H / 4 lanes walk one
    const int64_t chunks = (kmax + DET_CHUNK - 1) / DET_CHUNK;
    const dim3 grid((unsigned)((chunks + gpb - 1) / gpb), (unsigned)count);
    hipLaunchKernelGGL(det_scatter_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, pp);
    hipLaunchKernelGGL(det_scatter_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, pp);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int launch_det_keys3(void *stream, const DetKeys3 &q, int64_t total, int32_t *keys, int32_t *pos) {
    hipLaunchKernelGGL(det_keys3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, q, keys, pos);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int launch_det_iota(void *stream, int32_t *iota, int64_t n) {
    hipLaunchKernelGGL(det_iota_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, iota, n);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

}  // namespace pn
