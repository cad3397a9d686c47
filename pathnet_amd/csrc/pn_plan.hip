// pn_plan.hip -- the aggregator's index kernels on gfx950: the index plan (which table row every path step reads), the
// touched-row compaction of the distance bank, the stand-alone row gather (pn_pagg_gather), the padded copy of X for fc0's
// weight gradient and the zero fill of a backward's accumulators.  Launch parameters and launchers: pn_plan.h.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pn_internal.h"
#include "pn_kernels.h"
#include "pn_plan.h"

using namespace pn;

namespace {

// ================================================================================================
// index plan (the reference's view/flip/transposes collapsed into index arithmetic)
//   slot' = group * W + member is the order every later kernel uses (pooling groups contiguous).
//   original sequence slot q:  HOMO/PAGG q = slot'            (group = q / W)
//                              HETERO    q = member * S + group  (h_n.view(W, S, H), PathNet_run.py:196-197)
//   step t of slot q reads   HOMO/PAGG node ids[q, t]
//                            HETERO    r = q*L + t, node ids[r % P, L-1 - r / P]  (flip + reshape, :182-183)
//   and always the code codes[q, t] (:184 / :248).
// ================================================================================================
// (PlanDims: pn_plan.h)
__device__ __forceinline__ void plan_entry(int variant, const int32_t *ids, const uint8_t *codes, const PlanDims &d,
                                           int64_t slot, int t, int64_t &q, int &node, int &code) {
    if (variant == PN_VARIANT_HETERO) {
        const int64_t g = slot / d.W, mem = slot - g * d.W;
        q = mem * d.S_total + g;
        const int64_t r = q * d.L + t;
        node = ids[(r % d.P_total) * d.L + (d.L - 1 - (int)(r / d.P_total))];
    } else {
        q = slot;
        node = ids[(q - d.row_base) * d.L + t];
    }
    code = codes[(q - d.row_base) * d.L + t];
}

// slots [slot_begin, slot_begin + count) of the batch -> rowidx / egoidx / slotof of the local slots 0 .. count-1
// rank: null (row of the full table: node * L + code) or the compact row of (code, node) -- compact_rows below
__global__ void plan_kernel(int variant, const int32_t *__restrict__ ids, const uint8_t *__restrict__ codes, PlanDims d,
                            int64_t slot_begin, int64_t count, const int32_t *__restrict__ rank, int32_t *__restrict__ rowidx,
                            int32_t *__restrict__ egoidx, int32_t *__restrict__ slotof) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count * d.L) return;
    const int64_t ls = i / d.L;
    const int t = (int)(i - ls * d.L);
    int64_t q;
    int node, code;
    plan_entry(variant, ids, codes, d, slot_begin + ls, t, q, node, code);
    node = min(max(node, 0), d.N - 1);
    code = min(code, d.L - 1);
    const int32_t row = rank ? rank[(int64_t)code * d.N + node] : node * d.L + code;
    rowidx[i] = row;
    if (t == 0) {
        slotof[ls] = (int32_t)q;      // position in the whole batch: what the dropout counters / explicit masks index
        // attention ego: HOMO uses the transformed row of (q, step 0) (ego_full, :259-260);
        // HETERO uses the untransformed Xh row of path q's first node (neis[0], :199)
        egoidx[ls] = variant == PN_VARIANT_HETERO ? min(max(ids[(q - d.row_base) * d.L], 0), d.N - 1) : row;
    }
}

// ---- touched-row compaction ---------------------------------------------------------------------------------------------
// The distance bank is applied to (node, code) rows, N * L of them, whatever the batch reads (bank-before-gather, DESIGN.md
// section 4).  When the batch's path steps cannot touch half of them (a 10 M-node graph with 100 000 masked nodes: 24 M path
// steps, 60 M rows) the bank, its backward and the tables Z / dZ themselves shrink to the rows that ARE touched:
//   flags[code * N + node] = 1 for every path step (mark_rows_kernel), exclusive scan -> rank, the compact row of every
//   touched (code, node); list[compact row] = node; seg[c] = first compact row of code c (the rows are code-major, so each
//   code's rows are one contiguous GEMM against that code's weights); the index plan writes compact rows.
__global__ void mark_rows_kernel(int variant, const int32_t *__restrict__ ids, const uint8_t *__restrict__ codes, PlanDims d,
                                 int64_t slot_begin, int64_t count, uint8_t *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count * d.L) return;
    const int64_t ls = i / d.L;
    int64_t q;
    int node, code;
    plan_entry(variant, ids, codes, d, slot_begin + ls, (int)(i - ls * d.L), q, node, code);
    flags[(int64_t)min(code, d.L - 1) * d.N + min(max(node, 0), d.N - 1)] = 1;
}
// (SCAN_BLOCK, flags per workgroup: pn_plan.h)
__global__ __launch_bounds__(256) void scan_count_kernel(const uint8_t *__restrict__ flags, int64_t n, int32_t *__restrict__ bsum) {
    __shared__ int red[4];
    const int64_t base = (int64_t)blockIdx.x * SCAN_BLOCK + threadIdx.x * 16;
    int c = 0;
    if (base + 16 <= n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(flags + base);
        c = __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);        // (flags are 0 / 1 bytes)
    } else {
        for (int k = 0; k < 16; k++) c += base + k < n ? flags[base + k] : 0;
    }
    c = (int)wave_sum((float)c);        // <= 1024 per wave: exact in fp32
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) bsum[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
// exclusive scan of the block counts in place (one workgroup walks them: <= 15 k blocks for 60 M rows); total -> seg[L]
__global__ __launch_bounds__(1024) void scan_blocks_kernel(int32_t *__restrict__ bsum, int nb, int32_t *__restrict__ total) {
    __shared__ int part[1024];
    const int per = (nb + 1023) / 1024, lo = threadIdx.x * per, hi = min(nb, lo + per);
    int s = 0;
    for (int i = lo; i < hi; i++) s += bsum[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int i = 0; i < 1024; i++) {
            const int v = part[i];
            part[i] = run;
            run += v;
        }
        *total = run;
    }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int i = lo; i < hi; i++) {
        const int v = bsum[i];
        bsum[i] = run;
        run += v;
    }
}
__global__ __launch_bounds__(256) void scan_rank_kernel(const uint8_t *__restrict__ flags, int64_t n, int N, int L,
                                                        const int32_t *__restrict__ bsum, int32_t *__restrict__ rank,
                                                        int32_t *__restrict__ list, int32_t *__restrict__ seg) {
    __shared__ int wsum[4];
    const int64_t base = (int64_t)blockIdx.x * SCAN_BLOCK + threadIdx.x * 16;
    uint8_t f[16];
    int c = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        f[k] = base + k < n ? flags[base + k] : 0;
        c += f[k];
    }
    // exclusive scan of the 256 per-thread counts: inside the wave by shuffles, across the four waves through LDS
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int run = bsum[blockIdx.x] + inc - c;
    for (int w = 0; w < wave; w++) run += wsum[w];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const int64_t i = base + k;
        if (i < n) {
            rank[i] = run;
            const int code = (int)(i / N), node = (int)(i - (int64_t)code * N);
            if (node == 0) seg[code] = run;         // first row of a code (rows are code-major)
            if (f[k]) list[run] = node;
            run += f[k];
        }
    }
}

// rows[slot', t, :] = table[rowidx, :]   (stand-alone gather, also the HBM-roofline microbenchmark)
template <int VEC>
__global__ __launch_bounds__(256) void gather_kernel(int variant, const float *__restrict__ table,
                                                     const int32_t *__restrict__ ids,
                                                     const uint8_t *__restrict__ codes, PlanDims d, int64_t slot_begin,
                                                     int64_t count, int H, float *__restrict__ rows) {
    const int hv = H / VEC;
    const int64_t total = count * d.L * hv;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / hv;
        const int c = (int)(i - row * hv);
        const int64_t ls = row / d.L;
        const int t = (int)(row - ls * d.L);
        int64_t q;
        int node, code;
        plan_entry(variant, ids, codes, d, slot_begin + ls, t, q, node, code);
        node = min(max(node, 0), d.N - 1);
        code = min(code, d.L - 1);
        const int64_t src = ((int64_t)node * d.L + code) * hv + c;
        if (VEC == 4)
            reinterpret_cast<float4 *>(rows)[i] = reinterpret_cast<const float4 *>(table)[src];
        else
            rows[i] = table[src];
    }
}

// out [R][F4] = in [R][F] with zeros in columns F .. F4 - 1 (F4 = F rounded up to 4): 16-byte stores, dword loads
__global__ __launch_bounds__(256) void pad_rows_kernel(const float *__restrict__ in, int64_t R, int F, int F4, float *__restrict__ out) {
    const int q4 = F4 / 4;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= R * q4) return;
    const int64_t r = i / q4;
    const int c = (int)(i - r * q4) * 4;
    const float *src = in + r * F + c;
    float4 v;
    v.x = src[0];                       // (c < F always)
    v.y = c + 1 < F ? src[1] : 0.0f;
    v.z = c + 2 < F ? src[2] : 0.0f;
    v.w = c + 3 < F ? src[3] : 0.0f;
    reinterpret_cast<float4 *>(out)[i] = v;
}

// zero-fill of up to 12 buffers in one launch (the accumulated gradients of a backward; ZeroList / ZeroFill: pn_internal.h)
__global__ __launch_bounds__(256) void zero_kernel(ZeroList z) {
    for (int b = 0; b < z.n; b++) {
        float *p = z.ptr[b];
        const unsigned long long cnt = z.count[b];
        // 16-byte stores on the aligned body, scalars on the ragged ends
        const unsigned long long head = min(cnt, (unsigned long long)((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / 4);
        const unsigned long long body4 = (cnt - head) / 4;
        float4 *p4 = reinterpret_cast<float4 *>(p + head);
        for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < body4;
             i += (unsigned long long)gridDim.x * blockDim.x)
            p4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (blockIdx.x == 0) {
            for (unsigned long long i = threadIdx.x; i < head; i += blockDim.x) p[i] = 0.0f;
            for (unsigned long long i = head + body4 * 4 + threadIdx.x; i < cnt; i += blockDim.x) p[i] = 0.0f;
        }
    }
}

}  // namespace

namespace pn {

int launch_plan(void *stream, const PlanSteps &p, const int32_t *rank, int32_t *rowidx, int32_t *egoidx, int32_t *slotof) {
    const int64_t n = p.count * p.d.L;
    hipLaunchKernelGGL(plan_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p.variant, p.ids, p.codes,
                       p.d, p.slot_begin, p.count, rank, rowidx, egoidx, slotof);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int launch_compact_rows(void *stream, const PlanSteps &p, const CompactRows &out) {
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = p.count * p.d.L, rows = (int64_t)p.d.N * p.d.L;
    PN_CHECK_HIP(hipMemsetAsync(out.flags, 0, (size_t)rows, s));
    hipLaunchKernelGGL(mark_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p.variant, p.ids, p.codes, p.d,
                       p.slot_begin, p.count, out.flags);
    const int nb = (int)scan_block_count(rows);
    hipLaunchKernelGGL(scan_count_kernel, dim3(nb), dim3(256), 0, s, out.flags, rows, out.bsum);
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(1024), 0, s, out.bsum, nb, out.seg + p.d.L);
    hipLaunchKernelGGL(scan_rank_kernel, dim3(nb), dim3(256), 0, s, out.flags, rows, p.d.N, p.d.L, out.bsum, out.rank, out.list,
                       out.seg);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int launch_pad_rows(void *stream, const float *in, int64_t R, int F, int F4, float *out) {
    const int64_t n4 = R * (F4 / 4);
    hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, R, F, F4, out);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

}  // namespace pn

int pn::ZeroFill::flush(void *stream, bool timed) {
    if (!zl.n) return PN_OK;
    StageTimer tm(timed ? ctx : nullptr, ST_ZERO_FILL, stream);       // (d Z and d Xh are the bulk: rows of the graph, not paths)
    hipLaunchKernelGGL(zero_kernel, dim3(512), dim3(256), 0, (hipStream_t)stream, zl);
    PN_CHECK_HIP(hipGetLastError());
    zl.n = 0;
    return PN_OK;
}

extern "C" {

int pn_pagg_gather(pn_context *ctx, const pn_pagg_shape *shape, const float *table, const int32_t *ids,
                   const uint8_t *codes, float *rows, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!shape || !table || !ids || !codes || !rows) PN_FAIL(PN_ERR_ARG, "pn_pagg_gather: null");
    if (int rc = context_check_device(ctx)) return rc;
    const pn_pagg_shape &s = *shape;
    if (s.S < 0 || s.W < 1 || s.L < 1 || s.H < 1 || s.N < 1) PN_FAIL(PN_ERR_ARG, "pn_pagg_gather: bad shape");
    const int S_total = s.S_total > 0 ? s.S_total : s.S;
    if (s.group_begin < 0 || (int64_t)s.group_begin + s.S > S_total) PN_FAIL(PN_ERR_ARG, "pn_pagg_gather: bad slice");
    const int64_t count = (int64_t)s.S * s.W, rowsn = count * s.L;
    if (rowsn == 0) return PN_OK;
    const bool vec = (s.H % 4 == 0) && ((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(rows)) % 16 == 0);
    const int64_t work = rowsn * (vec ? s.H / 4 : s.H);
    const int blocks = (int)std::min<int64_t>((work + 255) / 256, 256 * 32);
    const PlanDims pd{S_total, s.W, s.L, s.N, (int64_t)S_total * s.W, 0};
    const int64_t slot_begin = (int64_t)s.group_begin * s.W;
    StageTimer tm(ctx, ST_GATHER, stream);
    if (vec)
        hipLaunchKernelGGL(gather_kernel<4>, dim3(blocks), dim3(256), 0, stream, s.variant, table, ids, codes, pd,
                           slot_begin, count, s.H, rows);
    else
        hipLaunchKernelGGL(gather_kernel<1>, dim3(blocks), dim3(256), 0, stream, s.variant, table, ids, codes, pd,
                           slot_begin, count, s.H, rows);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

}  // extern "C"
