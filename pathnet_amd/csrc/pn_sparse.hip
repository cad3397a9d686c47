// pn_sparse.hip -- fc0 for bag-of-words features: the non-zeros of X [N, F], extracted ONCE per feature matrix into a CSR and a
// CSC index (pn_sparse_count / pn_sparse_fill), and the two kernels that use them in place of the dense GEMMs -- the forward
// Xh = act(X . fc0_w^T + fc0_b) over the rows, the weight gradient g_fc0_w = dXh'^T . X over the columns.  Cora's X is 98.7 %
// zeros: 49 000 non-zeros x 128 outputs are 6 M FMAs where the dense kernels issue 500 M.
//
// Every sum is taken in a fixed order (rows: ascending feature, columns: four interleaved partial sums added in wavefront order), so
// the route serves the deterministic mode as it is.  An element counts as a non-zero when x != 0.0f: -0.0f does not, NaN and
// Inf do.  The one place the routes differ: 0 * (a non-finite weight) is NaN on the dense route and absent here.
#include <hip/hip_runtime.h>

#include "pn_sparse.h"

namespace pn {
namespace {

__device__ __forceinline__ int wave_bcast(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ float wave_bcast(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// ---- building the index ---------------------------------------------------------------------------------------------------
// row counts: one wavefront per row, to off[n + 1]
__global__ __launch_bounds__(256) void sp_count_rows_kernel(const float *__restrict__ X, int N, int F, int32_t *__restrict__ row_off) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const float *x = X + (int64_t)n * F;
    int cnt = 0;
    for (int f = lane; f < F; f += 64) cnt += x[f] != 0.0f ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) row_off[n + 1] = cnt;
}

// column counts: one lane per column walks the rows (256-byte loads per wavefront), to off[f + 1]
__global__ __launch_bounds__(64) void sp_count_cols_kernel(const float *__restrict__ X, int N, int F, int32_t *__restrict__ col_off) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= F) return;
    const float *x = X + f;
    int cnt = 0;
#pragma unroll 8
    for (int n = 0; n < N; n++) cnt += x[(int64_t)n * F] != 0.0f ? 1 : 0;
    col_off[f + 1] = cnt;
}

// off[0] = 0, off[1 .. n] = running sums of the counts stored there: one workgroup, 4 096 counts per round (workgroup y = 0
// takes the rows' array, 1 the columns')
__global__ __launch_bounds__(1024) void sp_scan_kernel(int32_t *__restrict__ off_a, int na, int32_t *__restrict__ off_b, int nb) {
    __shared__ int wsum[16];
    int32_t *off = blockIdx.x == 0 ? off_a : off_b;
    const int n = blockIdx.x == 0 ? na : nb;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int base = 0; base < n; base += 4096) {
        const int i = base + tid * 4;
        int v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = i + u < n ? off[1 + i + u] : 0;
        const int t = v[0] + v[1] + v[2] + v[3];
        int incl = t;
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < 16; w++) {
            const int s = wsum[w];
            if (w < wave) before += s;
            total += s;
        }
        int run = carry + before + incl - t;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            run += v[u];
            if (i + u < n) off[1 + i + u] = run;
        }
        carry += total;
        __syncthreads();
    }
    if (tid == 0) off[0] = 0;
}

// CSR: one wavefront per row; the position of a non-zero is the row's offset plus the number of non-zeros in front of it
// (ballot and prefix count), so features ascend.  A position past the row's end is not written; the counts and the fill must see
// the same X (the caller zero-fills the arrays, so a write to X in between leaves zeros, not uninitialised indices).
__global__ __launch_bounds__(256) void sp_fill_rows_kernel(const float *__restrict__ X, int N, int F, const int32_t *__restrict__ row_off,
                                                            int32_t *__restrict__ col, float *__restrict__ val) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const float *x = X + (int64_t)n * F;
    int at = row_off[n];
    const int end = row_off[n + 1];
    for (int f0 = 0; f0 < F; f0 += 64) {
        const int f = f0 + lane;
        const float v = f < F ? x[f] : 0.0f;
        const bool nz = v != 0.0f;
        const unsigned long long m = __ballot(nz);
        const int pos = at + __popcll(m & ((1ull << lane) - 1ull));
        if (nz && pos < end) {
            col[pos] = f;
            val[pos] = v;
        }
        at += __popcll(m);
    }
}

// CSC: one lane per column walks the rows in order, so nodes ascend
__global__ __launch_bounds__(64) void sp_fill_cols_kernel(const float *__restrict__ X, int N, int F, const int32_t *__restrict__ col_off,
                                                           int32_t *__restrict__ row, float *__restrict__ valc) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= F) return;
    const float *x = X + f;
    int at = col_off[f];
    const int end = col_off[f + 1];
#pragma unroll 8
    for (int n = 0; n < N; n++) {
        const float v = x[(int64_t)n * F];
        if (v != 0.0f && at < end) {
            row[at] = n;
            valc[at] = v;
            at++;
        }
    }
}

// ---- forward: a wavefront owns a node, lane l the output columns l, l + 64, ... (NJ of them: H <= 64 * NJ) -------------------
// The row's (feature, value) pairs are loaded 64 at a time, one pair per lane, and handed round; every pair reads one row of
// W0T [F, H] -- 4 * H contiguous bytes.  Eight pairs at a time: their rows' loads are in flight together (a short group loads
// its last pair again and leaves it out of the sum), the FMAs keep the order of the pairs.
constexpr int SP_GROUP = 8;
template <int NJ>
__global__ __launch_bounds__(256) void sparse_fc0_fwd_kernel(const int32_t *__restrict__ row_off, const int32_t *__restrict__ col,
                                                              const float *__restrict__ val, const float *__restrict__ W0T,
                                                              const float *__restrict__ bias, int N, int H, int relu,
                                                              uint32_t *__restrict__ clear_word, float *__restrict__ Xh) {
    if (clear_word && blockIdx.x == 0 && threadIdx.x == 0) clear_word[0] = clear_word[1] = clear_word[2] = 0u;
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const int b = __builtin_amdgcn_readfirstlane(row_off[n]), e = __builtin_amdgcn_readfirstlane(row_off[n + 1]);
    float acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) acc[j] = 0.0f;
    for (int c0 = b; c0 < e; c0 += 64) {
        const int cnt = min(64, e - c0);
        int cl = 0;
        float vl = 0.0f;
        if (lane < cnt) {
            cl = col[c0 + lane];
            vl = val[c0 + lane];
        }
        for (int k = 0; k < cnt; k += SP_GROUP) {
            float w[SP_GROUP][NJ], v[SP_GROUP];
#pragma unroll
            for (int u = 0; u < SP_GROUP; u++) {
                const int kk = min(k + u, cnt - 1);
                const float *wr = W0T + (size_t)wave_bcast(cl, kk) * H;
                v[u] = wave_bcast(vl, kk);
#pragma unroll
                for (int j = 0; j < NJ; j++) w[u][j] = j * 64 + lane < H ? wr[j * 64 + lane] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < SP_GROUP; u++)
                if (k + u < cnt) {
#pragma unroll
                    for (int j = 0; j < NJ; j++) acc[j] = fmaf(v[u], w[u][j], acc[j]);
                }
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const int h = j * 64 + lane;
        if (h < H) {
            float y = acc[j] + bias[h];
            if (relu) y = fmaxf(y, 0.0f);
            Xh[(size_t)n * H + h] = y;
        }
    }
}

// The bias gradient's workgroups (behind the features' in the weight-gradient launch; g_b given: the default mode): 64 rows
// of dXh' each, added to the zero-filled g_b with one atomic per column -- what colsum_kernel does with its row chunks.
constexpr int SP_BIAS_ROWS = 64;
template <int NJ>
__device__ __forceinline__ void sparse_bias_block(float (*part)[NJ * 64], int block, const float *__restrict__ dXh,
                                                  const float *__restrict__ gate, int N, int H, float *__restrict__ g_b) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = block * SP_BIAS_ROWS + wave * (SP_BIAS_ROWS / 4);
    float d[SP_BIAS_ROWS / 4][NJ];
#pragma unroll
    for (int u = 0; u < SP_BIAS_ROWS / 4; u++) {
        const size_t at = (size_t)min(r0 + u, N - 1) * H;
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const int h = j * 64 + lane;
            d[u][j] = h < H ? dXh[at + h] : 0.0f;
            if (gate && h < H && !(gate[at + h] > 0.0f)) d[u][j] = 0.0f;
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        float s = 0.0f;
#pragma unroll
        for (int u = 0; u < SP_BIAS_ROWS / 4; u++)
            if (r0 + u < N) s += d[u][j];
        part[wave][j * 64 + lane] = s;
    }
    __syncthreads();
    for (int h = threadIdx.x; h < H; h += 256) atomicAdd(g_b + h, ((part[0][h] + part[1][h]) + part[2][h]) + part[3][h]);
}

// ---- weight gradient: one workgroup per feature; wavefront w sums the entries w, w + 4, ... of the column in ascending node
// order (eight entries at a time, as in the forward), the four partial sums are added in the order ((0 + 1) + 2) + 3 through LDS
// and the column of g_w [H, F] is stored once (an empty column: zeros).  (A wavefront per feature with the same four partial
// sums was measured beside it: equal in the step, 2 x slower with the chip to itself -- profiles/sparse_fc0.txt section 4.)
template <int NJ>
__global__ __launch_bounds__(256) void sparse_fc0_wgrad_kernel(const int32_t *__restrict__ col_off, const int32_t *__restrict__ row,
                                                                      const float *__restrict__ valc, const float *__restrict__ dXh,
                                                                      const float *__restrict__ gate, int N, int F, int H,
                                                                      int feature_blocks, float *__restrict__ g_w,
                                                                      float *__restrict__ g_b) {
    __shared__ float part[4][NJ * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((int)blockIdx.x >= feature_blocks) {
        sparse_bias_block<NJ>(part, (int)blockIdx.x - feature_blocks, dXh, gate, N, H, g_b);
        return;
    }
    const int f = blockIdx.x;
    const int b = __builtin_amdgcn_readfirstlane(col_off[f]), e = __builtin_amdgcn_readfirstlane(col_off[f + 1]);
    const int mine = (e - b - wave + 3) / 4;        // entries b + wave + 4 * i, i < mine
    float acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) acc[j] = 0.0f;
    for (int i0 = 0; i0 < mine; i0 += 64) {
        const int cnt = min(64, mine - i0);
        int rl = 0;
        float vl = 0.0f;
        if (lane < cnt) {
            const int at = b + wave + 4 * (i0 + lane);
            rl = row[at];
            vl = valc[at];
        }
        for (int k = 0; k < cnt; k += SP_GROUP) {
            float d[SP_GROUP][NJ], v[SP_GROUP];
#pragma unroll
            for (int u = 0; u < SP_GROUP; u++) {
                const int kk = min(k + u, cnt - 1);
                const size_t at = (size_t)wave_bcast(rl, kk) * H;
                v[u] = wave_bcast(vl, kk);
#pragma unroll
                for (int j = 0; j < NJ; j++) {
                    const int h = j * 64 + lane;
                    d[u][j] = h < H ? dXh[at + h] : 0.0f;
                    if (gate && h < H && !(gate[at + h] > 0.0f)) d[u][j] = 0.0f;
                }
            }
#pragma unroll
            for (int u = 0; u < SP_GROUP; u++)
                if (k + u < cnt) {
#pragma unroll
                    for (int j = 0; j < NJ; j++) acc[j] = fmaf(v[u], d[u][j], acc[j]);
                }
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; j++) part[wave][j * 64 + lane] = acc[j];
    __syncthreads();
    for (int h = threadIdx.x; h < H; h += 256) g_w[(size_t)h * F + f] = ((part[0][h] + part[1][h]) + part[2][h]) + part[3][h];
}

int check_features(const pn_sparse_features &sp, int H, const char *who) {
    if (H < 32 || H > 256 || H % 32 != 0) PN_FAIL(PN_ERR_ARG, "%s: hidden size %d (multiples of 32 up to 256)", who, H);
    if (sp.nnz < 0 || !sp.row_off || !sp.col_off || (sp.nnz > 0 && (!sp.col || !sp.val || !sp.row || !sp.valc)))
        PN_FAIL(PN_ERR_ARG, "%s: incomplete sparse features", who);
    return PN_OK;
}

int check_matrix(const float *X, int32_t N, int32_t F, const char *who) {
    if (!X || N < 1 || F < 1) PN_FAIL(PN_ERR_ARG, "%s: bad matrix", who);
    if ((int64_t)N * F > SPARSE_MAX_ELEMS)
        PN_FAIL(PN_ERR_ARG, "%s: %lld elements, sparse features are prepared for at most 2^28", who, (long long)N * F);
    return PN_OK;
}

}  // namespace

int launch_sparse_fc0_fwd(hipStream_t stream, const pn_sparse_features &sp, int N, int H, const float *W0T, const float *bias,
                          int relu, uint32_t *clear_word, float *Xh) {
    if (int rc = check_features(sp, H, "sparse fc0 forward")) return rc;
    const dim3 grid((unsigned)((N + 3) / 4)), block(256);
#define PN_SP_FWD(NJ)                                                                                                       \
    hipLaunchKernelGGL(sparse_fc0_fwd_kernel<NJ>, grid, block, 0, stream, sp.row_off, sp.col, sp.val, W0T, bias, N, H, relu, \
                       clear_word, Xh)
    switch ((H + 63) / 64) {
        case 1: PN_SP_FWD(1); break;
        case 2: PN_SP_FWD(2); break;
        case 3: PN_SP_FWD(3); break;
        default: PN_SP_FWD(4); break;
    }
#undef PN_SP_FWD
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int launch_sparse_fc0_wgrad(hipStream_t stream, const pn_sparse_features &sp, int N, int F, int H, const float *dXh,
                            const float *gate, float *g_w, float *g_b) {
    if (int rc = check_features(sp, H, "sparse fc0 weight gradient")) return rc;
    const int feature_blocks = F, bias_blocks = g_b ? (N + SP_BIAS_ROWS - 1) / SP_BIAS_ROWS : 0;
    const dim3 grid((unsigned)(feature_blocks + bias_blocks)), block(256);
#define PN_SP_WGRAD(NJ)                                                                                                        \
    hipLaunchKernelGGL(sparse_fc0_wgrad_kernel<NJ>, grid, block, 0, stream, sp.col_off, sp.row, sp.valc, dXh, gate, N, F, H, \
                       feature_blocks, g_w, g_b)
    switch ((H + 63) / 64) {
        case 1: PN_SP_WGRAD(1); break;
        case 2: PN_SP_WGRAD(2); break;
        case 3: PN_SP_WGRAD(3); break;
        default: PN_SP_WGRAD(4); break;
    }
#undef PN_SP_WGRAD
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

}  // namespace pn

using namespace pn;

extern "C" {

int pn_sparse_count(pn_context *ctx, const float *X, int32_t N, int32_t F, int32_t *row_off, int32_t *col_off, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_matrix(X, N, F, "pn_sparse_count")) return rc;
    if (!row_off || !col_off) PN_FAIL(PN_ERR_ARG, "pn_sparse_count: null offsets");
    if (int rc = context_check_device(ctx)) return rc;
    hipLaunchKernelGGL(sp_count_rows_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, stream, X, N, F, row_off);
    hipLaunchKernelGGL(sp_count_cols_kernel, dim3((unsigned)((F + 63) / 64)), dim3(64), 0, stream, X, N, F, col_off);
    hipLaunchKernelGGL(sp_scan_kernel, dim3(2), dim3(1024), 0, stream, row_off, N, col_off, F);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

int pn_sparse_fill(pn_context *ctx, const float *X, int32_t N, int32_t F, const pn_sparse_features *sp, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_matrix(X, N, F, "pn_sparse_fill")) return rc;
    if (!sp) PN_FAIL(PN_ERR_ARG, "pn_sparse_fill: null features");
    if (int rc = check_features(*sp, 32, "pn_sparse_fill")) return rc;
    if (int rc = context_check_device(ctx)) return rc;
    if (sp->nnz == 0) return PN_OK;
    hipLaunchKernelGGL(sp_fill_rows_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, stream, X, N, F, sp->row_off,
                       sp->col, sp->val);
    hipLaunchKernelGGL(sp_fill_cols_kernel, dim3((unsigned)((F + 63) / 64)), dim3(64), 0, stream, X, N, F, sp->col_off,
                       sp->row, sp->valc);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

}  // extern "C"
