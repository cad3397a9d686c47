// pn_plan.h -- the aggregator's index kernels (pn_plan.hip): the index plan, the touched-row compaction, the stand-alone
// gather, and the two fills (padded copy of X, zero fill of the accumulated gradients).  Not part of the ABI.
#pragma once
#include <cstddef>
#include <cstdint>

#include "pn_internal.h"

namespace pn {

// A call may cover a slice of the batch (pn_pagg_shape: S_total, group_begin): `slot` below is the position in the WHOLE
// batch's slot' order, (group_begin + local group) * W + member; ids / codes are the whole batch's arrays.
struct PlanDims {
    int S_total, W, L, N;
    int64_t P_total;          // S_total * W
    int64_t row_base;         // batch position of row 0 of ids / codes (non-zero: the arrays hold a slice; HOMO / PAGG)
};

// the path steps a launch walks: steps 0 .. L-1 of the slots [slot_begin, slot_begin + count) of the batch
struct PlanSteps {
    int variant;
    const int32_t *ids;
    const uint8_t *codes;
    PlanDims d;
    int64_t slot_begin, count;
};

// rowidx [count, L] / egoidx [count] / slotof [count] of the local slots 0 .. count-1
// rank: null (row of the full table: node * L + code) or the compact row of (code, node) -- launch_compact_rows
int launch_plan(void *stream, const PlanSteps &p, const int32_t *rank, int32_t *rowidx, int32_t *egoidx, int32_t *slotof);

// touched-row compaction over the N * L (code, node) rows: flags (cleared here) -> rank / list / seg, seg[L] = their number
constexpr int SCAN_BLOCK = 256 * 16;        // flags per workgroup
inline size_t scan_block_count(int64_t rows) { return (size_t)((rows + SCAN_BLOCK - 1) / SCAN_BLOCK); }
struct CompactRows {
    uint8_t *flags;         // [N * L] (+ 16: the last workgroup's 16-byte load)
    int32_t *bsum;          // [scan_block_count(N * L) + 1]
    int32_t *rank;          // [N * L]
    int32_t *list;          // [touched rows]
    int32_t *seg;           // [L + 2]
};
int launch_compact_rows(void *stream, const PlanSteps &p, const CompactRows &out);

// out [R][F4] = in [R][F] with zeros in columns F .. F4 - 1 (F4 = F rounded up to 4)
int launch_pad_rows(void *stream, const float *in, int64_t R, int F, int F4, float *out);

// (the zero fill: ZeroFill::flush of pn_internal.h; pn_pagg_gather of the ABI launches the gather)

}  // namespace pn
