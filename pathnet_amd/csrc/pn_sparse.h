// pn_sparse.h -- fc0 over prepared sparse features (pn_sparse.hip): the forward and the weight gradient of the first linear
// layer for a feature matrix whose non-zeros were extracted once (pn_sparse_count / pn_sparse_fill).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pn_internal.h"

namespace pn {

// prepared features are taken for matrices of at most this many elements (positions stay in int32, the scans stay cheap)
constexpr int64_t SPARSE_MAX_ELEMS = (int64_t)1 << 28;

// Xh[n, :] = act(bias + sum_k val_k * W0T[col_k, :]) over the CSR rows, fp32 FMAs in ascending feature order; a row without
// non-zeros gives act(bias).  W0T [F, H] is the transposed weight; H: a multiple of 32 up to 256.  clear_word (or null): three
// words set to 0 by one thread of the launch (GemmParams::clear_word: the dense launch's epilogue).
int launch_sparse_fc0_fwd(hipStream_t stream, const pn_sparse_features &sp, int N, int H, const float *W0T, const float *bias,
                          int relu, uint32_t *clear_word, float *Xh);
// g_w[h, f] = sum over the entries (n, v) of column f, in a fixed order, of v * dXh[n, h] * [gate[n, h] > 0] (gate may be null);
// every element of g_w [H, F] is stored once, empty columns as zeros.  g_b (or null): the bias gradient, the column sums of the
// gated dXh [N, H], is ADDED to it by extra workgroups of the same launch, row chunk by row chunk with fp32 atomics -- the
// default mode; a deterministic caller passes null and takes launch_colsum(det = true).
int launch_sparse_fc0_wgrad(hipStream_t stream, const pn_sparse_features &sp, int N, int F, int H, const float *dXh,
                            const float *gate, float *g_w, float *g_b);

}  // namespace pn
