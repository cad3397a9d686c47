// pn_det.h -- the deterministic scatter-add of the aggregator's backward (pn_det.hip; pn_pagg_shape.deterministic): sorted
// (destination, position) pairs walked in chunks, every destination row with one writer and a fixed order.  Not part of the ABI.
#pragma once
#include <cstdint>

#include "pn_internal.h"

namespace pn {

constexpr int DET_CHUNK = 32;
struct DetScatterParams {
    const int32_t *skey, *ssrc;     // sorted keys (with the scatter's segment number above `kmask`); the unsorted position of every one
    int32_t kmask;
    int64_t K, chunk0;              // positions; first chunk of this scatter's region of cpart
    const float *rows;              // [K, H] or null
    const float *scal, *vec;        // [K], [H]
    float *dst;                     // [., H]
    float *cpart;                   // [chunks][2][H]
    int H;
};

struct DetScatterPair {          // blockIdx.y picks the scatter: the pooling backward's two run in one launch
    DetScatterParams s[2];
};
// pass 1, then pass 2, of one scatter or of two that write different rows (blockIdx.y picks): two launches on `stream`
int launch_det_scatters(void *stream, const DetScatterParams *list, int count);

// keys of a scatter, clamped to [0, hi], beside the identity permutation the sort carries along
struct DetKeys3 {
    const int32_t *keys[3];
    int64_t n[3];
    int32_t hi[3];
    int shift;
};
// keys [total] = the three key arrays back to back, clamped, with the segment number above bit `shift`; pos = position in its segment
int launch_det_keys3(void *stream, const DetKeys3 &q, int64_t total, int32_t *keys, int32_t *pos);

// iota[i] = i, i < n: the identity the BPTT kernels index the contribution buffer with
int launch_det_iota(void *stream, int32_t *iota, int64_t n);

}  // namespace pn
