// pn_pagg.hip -- the path aggregator ("PAGG") forward and backward on gfx950.
//
// Replaces the forward() bodies of
//   PathNet       /root/reference/PathNet_run.py:172-211   (variant HETERO)
//   PathNet_homo  /root/reference/PathNet_run.py:239-278   (variant HOMO)
//   PAGG          /root/reference/baseline/GPRGNN/src/copy.py:327-359   (variant PAGG)
// and the autograd backward the reference gets from loss.backward() (PathNet_run.py:351).
//
// This file is the call's orchestration and holds no kernel: shapes (Dims), the workspace layout (WsLayout), one resolved call
// (Call), the stages run_* that fill the kernels' parameter structs from the workspace, choose streams and bracket the
// per-stage profile, pagg_backward_impl and the entry points of the ABI.  The kernels and their launchers:
//   pn_plan.hip   (pn_plan.h)   index plan, touched-row compaction, stand-alone gather (pn_pagg_gather), padded X, zero fill
//   pn_gemm.hip   (pn_gemm.h)   node-level GEMMs: fc0, distance bank, classifier, their gradients
//   pn_seqh.hip / pn_seq3.hip / pn_seq4.hip (pn_seq.h)   the fused recurrent kernels, fp16 x 2 and bf16 x 3 planes
//   pn_seqgen.hip (pn_seq.h)    mean / sum encoders, the step-by-step recurrence for hidden sizes above 256
//   pn_pool.hip   (pn_pool.h)   pooling forward / backward, the pooling step, loss sum, attention-weight reduce
//   pn_det.hip    (pn_det.h)    deterministic scatter-add
//   pn_rgrad.hip, pn_sparse.hip, pn_sort.hip, pn_train.hip   row-reduction weight gradients, sparse fc0, radix sort, loss
//
// How the reference's op sequence maps onto kernels
//   fc0 (+ReLU)                      :175 / :242-243      -> gemm_kernel (pn_gemm.hip)            Xh[N,H]
//   L Linear layers on P*L gathered rows, stack, select by distance code
//                                    :185-191 / :249-255  -> ONE gemm over the N nodes:
//        Z[v, d, :] = nets[d](Xh[v])  for every node v and code d  (N*L rows instead of P*L*L),
//        after which "gather + select" is a single row gather  Z[node(q,t)*L + code(q,t)].
//        Same dot products per emitted row, ~S*W*L/N times fewer FLOPs, no [P*L, L, H] temporary.
//   X[neis] gather, flip / view quirks :179-184 / :246     -> plan_kernel (pn_plan.hip; index plan only)
//   dropout, nn.LSTM / nn.RNN          :194-195 / :264-265 -> seq_fwdh_kernel (pn_seqh.hip, fp16 x 2 planes, the default) or
//        seq_fwd3_kernel (pn_seq3.hip, bf16 x 3): coalesced row gather into an LDS path tile, MFMA for
//        [x_t ; h_{t-1}] x [W_ih ; W_hh]^T, cell math in registers, h_t back to LDS, L steps without leaving the CU;
//        hidden sizes above 256: the step-by-step recurrence gen_*_kernel (pn_seqgen.hip)
//   attention over the W paths, mean, concat ego, dropout, fc2
//                                    :196-210 / :266-277  -> pool_fwd_kernel (pn_pool.hip): one workgroup per node, wave shuffles
//        for the per-path dot products and the reduction over W
//   loss.backward()                    :351                -> pool_bwd_wg_kernel (pn_pagg_train_step: pool_step_kernel = pooling
//        forward + cross entropy + pooling backward of a node in one launch), seq_bwdh / seq_bwd3 (BPTT + atomic scatter of the
//        gather backward), wgradh / wgrad3 / wgrad4 (dG^T . [x|h]), gemm_kernel for the bank / fc0 gradients; deterministic
//        mode: det_scatter_kernel (pn_det.hip) and fixed-order finishes instead of the atomics
//
// Precision: inputs, outputs, accumulation and all element-wise math are fp32.  The node-level GEMMs use the fp32-input MFMA
// (an exact FMA chain) or bf16 x 3 planes on large graphs; the three recurrent GEMMs evaluate every fp32 product on the 16-bit
// matrix pipe over exact plane splits of both operands (pn_kernels.h) -- the contract is 1e-5 on fp32 logits against the
// reference CPU path, tests measure 3e-7 against float64.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include "pn_det.h"
#include "pn_gemm.h"
#include "pn_internal.h"
#include "pn_loss.h"
#include "pn_plan.h"
#include "pn_pool.h"
#include "pn_seq.h"
#include "pn_sparse.h"

using namespace pn;

// Settled by measurement in rounds 1-4 and no longer build options (profiles/HISTORY_r1_r4.md): descending tile order in the BPTT,
// strided K tiles in the weight gradient, the attention-weight terms through per-workgroup partials (atomics serialised), one row
// block per wave in the forward (two: 0.411 vs 0.308 ms), no s_setprio around the MFMA phases, the independent small launches on the
// context's second stream.
namespace {

// ================================================================================================
// shape bookkeeping and workspace layout
// ================================================================================================
enum { CELL_LSTM = 1, CELL_RNN = 2, CELL_GRU = 3, CELL_MEAN = 4, CELL_SUM = 5 };   // = PN_CELL_*
struct Dims {
    int variant, N, F, H, C, S, W, L, G, SV;    // G: gate slots of the recurrent kernels (4: LSTM and GRU, 1: RNN, 0: mean / sum)
    int cell, Gw;                               // cell kind; Gw: gates of the caller's weight tensors (4, 1, 3, 0)
    int gru;                                    // 1: the cell is a GRU (its three gates are packed into the four slots)
    bool generic;                               // H > 256: the step-by-step recurrence (gen_*_kernel) instead of the fused kernels
    int S_total, group_begin;
    int Sb;             // pooling groups per micro-batch
    int nb;             // micro-batches of this call
    int64_t P_total;    // paths of the whole batch
    bool det;           // pn_pagg_shape.deterministic: the backward adds in a fixed order (no floating-point atomics)
    bool compact;       // the bank runs over the (node, code) rows this call's paths touch (compact_rows)
    int64_t ZR;         // rows of Z / dZ: N * L, or the bound of the touched rows
    int math;           // PN_SEQ_MATH_F16X2 / PN_SEQ_MATH_BF16X3 for the fused recurrent kernels, 0 when the call has none
};

int make_dims(const pn_pagg_shape &s, Dims &d) {
    if (s.variant < 0 || s.variant > 2) PN_FAIL(PN_ERR_ARG, "unknown variant %d", s.variant);
    if (s.H < 32 || s.H > 1024 || s.H % 32 != 0)
        PN_FAIL(PN_ERR_ARG, "hidden size %d not supported (multiples of 32 up to 1024; fused kernels up to 256)", s.H);
    if (s.N < 1 || s.F < 1 || s.C < 1 || s.S < 0 || s.W < 1 || s.L < 1 || s.L > 64)
        PN_FAIL(PN_ERR_ARG, "bad aggregator shape N=%d F=%d C=%d S=%d W=%d L=%d", s.N, s.F, s.C, s.S, s.W, s.L);
    // the pooling kernels keep per-walk scores, coefficients, ego rows and a few rows of H floats in LDS (pool_lds_bytes, pn_pool.hip:
    // linear in W, which gives the largest W the message names)
    if (pool_lds_bytes(s.W, s.H) > 64 * 1024) {
        const size_t at0 = pool_lds_bytes(0, s.H), per_walk = pool_lds_bytes(1, s.H) - at0;
        PN_FAIL(PN_ERR_ARG, "W=%d walks per node exceed the pooling kernels' LDS budget (W <= %d at H=%d)", s.W,
                (int)((64 * 1024 - at0) / per_walk), s.H);
    }
    if (s.variant == PN_VARIANT_PAGG && s.L != 4)
        PN_FAIL(PN_ERR_ARG, "PAGG has exactly four distance layers nei0..nei3 (copy.py:310-313); L=%d", s.L);
    if (s.cell < 0 || s.cell > CELL_SUM) PN_FAIL(PN_ERR_ARG, "unknown cell %d", s.cell);
    const int S_total = s.S_total > 0 ? s.S_total : s.S;
    if (s.group_begin < 0 || (int64_t)s.group_begin + s.S > S_total || s.batch_groups < 0)
        PN_FAIL(PN_ERR_ARG, "bad slice: groups [%d, +%d) of a batch of %d, batch_groups=%d", s.group_begin, s.S,
                S_total, s.batch_groups);
    // int32 indices: a node's table row (node * L + code) and a path's position in the batch
    if ((int64_t)S_total * s.W > 2000000000LL || (int64_t)s.N * s.L > 2000000000LL)
        PN_FAIL(PN_ERR_ARG, "index space exceeds int32 (S_total*W = %lld paths, N*L = %lld rows)",
                (long long)S_total * s.W, (long long)s.N * s.L);
    d.variant = s.variant;
    d.N = s.N, d.F = s.F, d.H = s.H, d.C = s.C, d.S = s.S, d.W = s.W, d.L = s.L;
    d.cell = s.cell ? s.cell : (s.variant == PN_VARIANT_PAGG ? CELL_RNN : CELL_LSTM);
    d.G = d.cell == CELL_RNN ? 1 : (d.cell == CELL_LSTM || d.cell == CELL_GRU) ? 4 : 0;
    d.gru = d.cell == CELL_GRU ? 1 : 0;
    d.Gw = d.gru ? 3 : d.G;
    d.SV = d.G == 4 ? 5 : 1;
    d.generic = s.H > 256 && d.G > 0;
    d.S_total = S_total;
    d.group_begin = s.group_begin;
    d.Sb = (s.batch_groups > 0 && s.batch_groups < s.S) ? s.batch_groups : s.S;
    d.nb = d.Sb > 0 ? (s.S + d.Sb - 1) / d.Sb : 1;
    d.P_total = (int64_t)S_total * s.W;
    d.det = s.deterministic != 0;
    {
        // compaction pays when the path steps of this call cannot touch half of the N * L rows (pn_pagg_shape.compact forces
        // it on / off: tests, A/B); the hetero class reads paths of the whole batch, a slice marks the whole batch's steps
        const int64_t steps = (int64_t)(d.variant == PN_VARIANT_HETERO ? S_total : s.S) * s.W * s.L, rows = (int64_t)s.N * s.L;
        if (s.compact < 0 || s.compact > PN_COMPACT_OFF) PN_FAIL(PN_ERR_ARG, "unknown compact mode %d", s.compact);
        d.compact = s.S > 0 && (s.compact == PN_COMPACT_AUTO ? 2 * steps < rows : s.compact == PN_COMPACT_ON);
        d.ZR = d.compact ? std::min(rows, steps) : rows;
    }
    if (s.seq_math < 0 || s.seq_math > PN_SEQ_MATH_F16X2) PN_FAIL(PN_ERR_ARG, "unknown seq_math %d", s.seq_math);
    d.math = (d.G > 0 && !d.generic) ? (s.seq_math == PN_SEQ_MATH_BF16X3 ? PN_SEQ_MATH_BF16X3 : PN_SEQ_MATH_F16X2) : 0;
    // rows of one micro-batch's [Pb * L, .] tensors are counted in int32 inside the kernels
    if ((int64_t)d.Sb * s.W * s.L > 2000000000LL)
        PN_FAIL(PN_ERR_ARG, "%lld path steps in one micro-batch exceed int32: set batch_groups", (long long)d.Sb * s.W * s.L);
    return PN_OK;
}

#ifndef PN_WGRAD_CUS_SHARED
#define PN_WGRAD_CUS_SHARED 224    // (tuning builds 176 .. 240: profiles/r06_glue.txt section 11 -- 208 won while fc0's weight
#endif                             //  gradient was a 150 us gemm_kernel launch beside it, 224 again once that ran on rgrad_kernel)
constexpr int WGRAD_CUS_SHARED = PN_WGRAD_CUS_SHARED;   // CUs of the weight-gradient launch when something is meant to run beside it (of 256)
// (a call over prepared sparse features keeps the same split: 232 .. 256 each lost ~30 us there, profiles/sparse_fc0.txt)
// fc0's weight gradient runs on rgrad_kernel (16-byte row loads) also when F is not a multiple of 4 -- Cora's 1433 -- from a
// copy of X with padded rows, made per backward (pad_rows_kernel: 2 x 15 MB at the headline shape, ~5 us, for a GEMM that
// takes 150 us on the 48 CUs the recurrent weight gradient leaves it and ~60 as a row reduction).  Graphs from 2 048 nodes
// on whose copy stays below 256 MB; floats of the copy, 0: no copy.
inline size_t xpad_floats(const Dims &d) {
    if (d.F % 4 == 0 || d.N < 2048 || d.det) return 0;
    const size_t f4 = (size_t)(d.F + 3) / 4 * 4, n = (size_t)d.N * f4;
    return n * 4 <= ((size_t)256 << 20) ? n : 0;
}

struct WsLayout {
    size_t Xh, Z, range, wmax;                                           // node tables (first: reuse_tables relies on it); partial weight maxima
    size_t Wp, biasc, WpT, wpart, gpart, dZ, dXh;                        // weights / node-level backward
    size_t rowidx, egoidx, slotof, hn, saved, coef, rawsc, layer1, outb; // per micro-batch, forward
    size_t xh, keep, dG, dhn, dl1, gx, gout, bankT, xpad;                // per micro-batch, saved / backward
    size_t flags, rank, list, seg, bsum;                                 // touched-row compaction (Dims.compact)
    size_t dx, keys, iota, skey, stmp, cpart, dsel, dds, datt, dgemm;  // deterministic backward (Dims.det)
    size_t okey, osrc;                  // its three destination orders, sorted once per micro-batch into one block each: segment
                                        // offsets are running sums over the segments present (det_params), nothing is laid out here
    size_t w0t;                         // fc0_w transposed [F, H]: the sparse forward reads its rows (last: appended to the layout)
    size_t stmp_bytes;
    int wgrad_split, wgrad_tiles;
    size_t total;
};

inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }

WsLayout ws_layout(const Dims &d) {
    WsLayout w{};
    const size_t N = d.N, H = d.H, L = d.L, G = d.G, SV = d.SV, Sb = d.Sb, Pb = (size_t)d.Sb * d.W;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        size_t o = at;
        at = align256(at + bytes);
        return o;
    };
    w.Xh = take(N * H * 4);
    w.Z = take((size_t)d.ZR * H * 4);
    w.range = take(sizeof(SeqRange));       // operand ranges of the fp16 recurrent kernels; range.x belongs to Z
    w.wmax = take(64 * 4);                  // partial maxima of |W_ih| / |W_hh| (range_part_kernel -> pack_fb_kernel)
    w.Wp = take(G * H * 3 * H * 4);          // (G = 0, the mean / sum encoders: no recurrent weights, no saved gates)
    w.biasc = take(G * H * 4);
    w.WpT = take(G * H * 3 * H * 4);
    {
        // split of the Pb*L rows of the weight-gradient GEMM: one 8-wave workgroup per CU.  Such a workgroup takes the CU's
        // whole register file: with one on every CU the node-level GEMMs of the main stream (bank / fc0 backward) cannot
        // start until the launch is over, whatever stream they are on.  A short launch (a Cora-sized batch: 0.17 ms against
        // ~0.07 ms of launch-bound GEMMs) therefore leaves an eighth of the CUs free -- the kernel is HBM-bound enough to
        // lose 3 % on 224 CUs, the step wins 2.8 % (0.988 -> 0.959 ms; re-measured in round 6); where the weight gradient is 6-12x the GEMM chain
        // (Pubmed, BGP size: +10 % on the kernel for nothing hidden) it keeps every CU.  profiles/r04_wgrad_cus_ab.txt
        const size_t rows = Pb * L, tiles = std::max<size_t>(1, ((G * H + WG_BM - 1) / WG_BM) * ((2 * H + WG_BN - 1) / WG_BN));
        const double wg_flops = 2.0 * (double)rows * (double)(G * H) * (double)(2 * H);
        size_t cus = wg_flops <= 1.2e11 ? WGRAD_CUS_SHARED : 256;
        size_t nz = (cus + tiles - 1) / tiles;
        const size_t max_nz = (rows + 4 * WG_KT - 1) / (4 * WG_KT);
        if (nz > max_nz) nz = max_nz;
        if (nz < 1) nz = 1;
        w.wgrad_split = (int)nz;
        w.wgrad_tiles = (int)tiles;
        w.wpart = take(nz * (G * H * 2 * H + G * H) * 4);
    }
    {
        const int nz = std::max(gemm_split_count(d.N, d.H, d.F), gemm_split_count(d.N, d.H, d.L * d.H));
        w.gpart = take(nz > 1 ? (size_t)nz * N * H * 4 : 0);
    }
    w.dZ = take((size_t)d.ZR * H * 4);
    w.dXh = take(N * H * 4);
    w.rowidx = take(Pb * L * 4);
    w.egoidx = take(Pb * 4);
    w.slotof = take(Pb * 4);
    w.hn = take(Pb * H * 4);
    w.saved = take(Pb * L * SV * H * 4);
    w.coef = take(Pb * 4);
    w.rawsc = take(Pb * 4);
    w.layer1 = take(Sb * 2 * H * 4);
    w.outb = take(Sb * (size_t)d.C * 4);
    w.xh = take(Pb * L * 2 * H * 4);
    w.keep = take(Pb * L * (H / 4));
    w.dG = take(Pb * L * G * H * 4);
    w.dhn = take(Pb * H * 4);
    w.dl1 = take(Sb * 2 * H * 4 + 1024);
    w.gx = take(d.generic ? Pb * 2 * H * 4 : 0);        // [dx_t | dh_{t-1}] of a step of the generic recurrence
    w.gout = take(Sb * (size_t)d.C * 4);                // d loss / d logits of a micro-batch (pn_pagg_train_step)
    w.datt = take(Sb * (2 * H + 4) * 4);                // per-workgroup attention-weight terms of the pooling backward
    w.bankT = take(L * H * H * 4);                      // transposed bank weights (the dX GEMM on the bf16 x 3 kernel)
    w.xpad = take(xpad_floats(d) * 4);                  // X with its rows padded to a multiple of four floats (fc0's weight gradient on rgrad_kernel)
    w.flags = take(d.compact ? N * L + 16 : 0);
    w.rank = take(d.compact ? N * L * 4 : 0);
    w.list = take(d.compact ? (size_t)d.ZR * 4 : 0);
    w.seg = take(d.compact ? (L + 2) * 4 : 0);
    w.bsum = take(d.compact ? (scan_block_count((int64_t)(N * L)) + 1) * 4 : 0);
    if (d.det) {
        // contributions of the gather backward ([Pb * L, H] rows), their (destination row, position) pairs before and
        // after the sort, the sort's temporary storage, the sums of the segments that cross a chunk boundary; the
        // pooling backward's per-group / per-path / per-workgroup terms; the chunk sums of the weight-gradient GEMMs
        const size_t K = std::max(Pb * L, Sb), C = d.C, F = d.F;
        w.dx = take(Pb * L * H * 4);
        // the three scatters' (destination, position) pairs are sorted TOGETHER (prepare_det_orders): keys / positions before the
        // sort (keys, skey), after it (okey / osrc: one block, a segment per scatter), the identity the BPTT indexes with (iota)
        const size_t ord[3] = {Sb, Pb, Pb * L};        // DET_SEL, DET_EGO, DET_ROW
        const size_t Kt = ord[0] + ord[1] + ord[2];
        w.keys = take(Kt * 4);
        w.iota = take(K * 4);
        w.skey = take(Kt * 4);
        w.okey = take(Kt * 4);
        w.osrc = take(Kt * 4);
        w.stmp_bytes = sort_temp_reserve((int64_t)Kt);
        w.stmp = take(w.stmp_bytes);
        w.cpart = take((Kt / DET_CHUNK + 4) * 2 * H * 4);      // (a region per scatter: SEL and EGO run in one launch)
        w.dsel = take(Sb * H * 4);
        w.dds = take(Pb * 4);
        w.dgemm = take(std::max({det_gemm_floats(C, 2 * H), det_gemm_floats(d.compact ? H : L * H, H), det_gemm_floats(H, F)}) * 4);
    }
    w.w0t = take(d.H <= 256 ? (size_t)d.F * H * 4 : 0);    // (sized by the shape alone: a call may or may not carry features)
    w.total = at;
    return w;
}

// Independent launches go to the context's second stream (pn_context.hip): the index plan and the weight packing beside
// fc0 / bank in the forward; in the backward the classifier's weight gradient beside the pooling backward and the
// BPTT, and the recurrent weight-gradient GEMM (one 8-wave workgroup per CU, 104 KB of LDS) beside the node-level
// GEMMs that follow the BPTT.  The guard makes `stream` wait for whatever was forked on every way out.
struct JoinGuard {
    pn_context *ctx;
    hipStream_t stream;
    bool pending = false;
    int mark() {                        // the forked work is complete up to here on the second stream
        if (int rc = context_record_join(ctx)) return rc;
        pending = true;
        return PN_OK;
    }
    int join() {
        if (!pending) return PN_OK;
        pending = false;
        return context_join(ctx, stream);
    }
    ~JoinGuard() { (void)join(); }
};

// ---- one aggregator call, resolved: shapes, workspace pointers, and the stages that run once per micro-batch ---------
struct Call {
    pn_context *ctx;
    hipStream_t stream;
    const pn_pagg_args *a;
    Dims d;
    WsLayout w;
    char *ws;
    const float *Xh;
    float *Z;
    const pn_sparse_features *sp;       // prepared features of a->X that this call uses for fc0, or null: the dense kernels
    const float *omega;                 // pn_path_weights.weight of the call, or null: the unweighted pooling
    int norm;                           // PN_PATH_NORM_*
    template <class T>
    T *at(size_t off) const { return reinterpret_cast<T *>(ws + off); }
    int groups(int b) const { return std::min(d.Sb, d.S - b * d.Sb); }                 // pooling groups of micro-batch b
    int64_t group0(int b) const { return (int64_t)d.group_begin + (int64_t)b * d.Sb; }  // its first group, batch-wide
    const int32_t *sel(int b) const { return a->sel + (a->index_rows_local ? (int64_t)b * d.Sb : group0(b)); }
};

int resolve_call(Call &c, pn_context *ctx, const pn_pagg_args *a, hipStream_t stream, const char *who,
                 const pn_sparse_features *sp = nullptr, const pn_path_weights *pw = nullptr) {
    if (!a) PN_FAIL(PN_ERR_ARG, "%s: null args", who);
    if (int rc = context_check_device(ctx)) return rc;
    if (int rc = make_dims(a->shape, c.d)) return rc;
    c.ctx = ctx;
    c.stream = stream;
    c.a = a;
    c.w = ws_layout(c.d);
    if (!a->workspace) PN_FAIL(PN_ERR_ARG, "%s: null workspace", who);
    if (a->workspace_bytes < (int64_t)c.w.total)
        PN_FAIL(PN_ERR_CAPACITY, "aggregator workspace holds %lld bytes, need %lld", (long long)a->workspace_bytes,
                (long long)c.w.total);
    c.ws = reinterpret_cast<char *>(a->workspace);
    c.Xh = a->Xh_in ? a->Xh_in : c.at<const float>(c.w.Xh);
    c.Z = c.at<float>(c.w.Z);
    // prepared features serve fc0 where the library runs it itself, at the fused hidden sizes; PN_FC0_SPARSE = 0 ignores them
    c.sp = (sp && !a->Xh_in && c.d.H <= 256 && (int64_t)c.d.N * c.d.F <= SPARSE_MAX_ELEMS && knobs_of(ctx).fc0_sparse != 0) ? sp : nullptr;
    c.omega = pw ? pw->weight : nullptr;
    c.norm = pw ? pw->norm : PN_PATH_NORM_SUM;
    if (c.norm != PN_PATH_NORM_SUM && c.norm != PN_PATH_NORM_COUNT) PN_FAIL(PN_ERR_ARG, "%s: unknown pn_path_weights.norm %d", who, c.norm);
    if (a->index_rows_local && c.d.variant == PN_VARIANT_HETERO && (c.d.group_begin != 0 || c.d.S != c.d.S_total))
        PN_FAIL(PN_ERR_ARG, "%s: the hetero class reads paths of the whole batch (PathNet_run.py:196-197): "
                "index_rows_local needs the whole batch's ids / codes", who);
    return PN_OK;
}

// the path steps of the batch's slots [slot_begin, slot_begin + count), as the index kernels walk them
inline PlanSteps plan_steps(const Call &c, int64_t slot_begin, int64_t count) {
    const Dims &d = c.d;
    const PlanDims pd{d.S_total, d.W, d.L, d.N, d.P_total, c.a->index_rows_local ? (int64_t)d.group_begin * d.W : 0};
    return PlanSteps{d.variant, c.a->ids, c.a->codes, pd, slot_begin, count};
}

int run_plan(const Call &c, hipStream_t s, int b) {
    const Dims &d = c.d;
    return launch_plan(s, plan_steps(c, c.group0(b) * d.W, (int64_t)c.groups(b) * d.W),
                       d.compact ? c.at<const int32_t>(c.w.rank) : nullptr, c.at<int32_t>(c.w.rowidx), c.at<int32_t>(c.w.egoidx),
                       c.at<int32_t>(c.w.slotof));
}

// flags -> rank / list / seg for the (node, code) rows this call's paths touch (the hetero class: the whole batch's)
int run_compact_rows(const Call &c, hipStream_t s) {
    const Dims &d = c.d;
    const bool het = d.variant == PN_VARIANT_HETERO;
    const int64_t slot0 = het ? 0 : (int64_t)d.group_begin * d.W, count = (int64_t)(het ? d.S_total : d.S) * d.W;
    return launch_compact_rows(s, plan_steps(c, slot0, count),
                               CompactRows{c.at<uint8_t>(c.w.flags), c.at<int32_t>(c.w.bsum), c.at<int32_t>(c.w.rank),
                                           c.at<int32_t>(c.w.list), c.at<int32_t>(c.w.seg)});
}

// ---- the generic recurrence (H > 256): step-by-step kernels + the fp32 GEMM ------------------------------------------
GenParams gen_params(const Call &c, int b) {
    const Dims &d = c.d;
    const pn_pagg_args *a = c.a;
    GenParams gp{};
    gp.Z = c.Z;
    gp.rowidx = c.at<int32_t>(c.w.rowidx);
    gp.slotof = c.at<int32_t>(c.w.slotof);
    gp.xh = c.at<float>(c.w.xh);
    gp.pre = c.at<float>(c.w.dG);
    gp.hn = c.at<float>(c.w.hn);
    gp.gx = c.at<float>(c.w.gx);
    gp.dZ = c.at<float>(c.w.dZ);
    gp.biasc = c.at<float>(c.w.biasc);
    gp.P = c.groups(b) * d.W;
    gp.L = d.L;
    gp.H = d.H;
    gp.G = d.G;
    gp.cell = d.cell;
    gp.Pmask = d.P_total;
    gp.p_drop = a->p_seq;
    gp.seed = a->seed;
    gp.dyn = a->step_state;
    gp.mask = a->mask_seq;
    return gp;
}

int run_seq_fwd_generic(const Call &c, int b, bool save) {
    const Dims &d = c.d;
    GenParams gp = gen_params(c, b);
    gp.saved = save ? c.at<float>(c.w.saved) : nullptr;
    gp.state = c.at<float>(c.w.dhn);            // (a backward-only buffer: the running cell / hidden state lives there)
    const int H = d.H, GH = d.G * H, P = gp.P;
    const float *Wcat = c.at<const float>(c.w.Wp);
    StageTimer tm(c.ctx, ST_SEQ_FWD, c.stream);
    for (int t = 0; t < d.L; t++) {
        gp.t = t;
        if (int rc = launch_gen_x(c.stream, gp)) return rc;
        // pre[q, :] = [x_t | h_{t-1}] . Wcat^T + b      (step 0: h_{-1} = 0, the x half of K suffices)
        GemmParams g = gemm_linear_fwd(gp.xh + (size_t)t * 2 * H, (int64_t)d.L * 2 * H, Wcat, 2 * H, gp.pre + (size_t)t * GH,
                                       (int64_t)d.L * GH, P, t == 0 ? H : 2 * H, GH);
        g.bias = gp.biasc;
        if (int rc = launch_gemm3(c.stream, gemm3_of(g))) return rc;
        if (int rc = launch_gen_cell_fwd(c.stream, gp)) return rc;
    }
    return PN_OK;
}

// BPTT of micro-batch b (the weight gradient dG^T . [x | h] is the fused path's wgrad3_kernel: it has no size limit)
int run_seq_bwd_generic(const Call &c, int b) {
    const Dims &d = c.d;
    GenParams gp = gen_params(c, b);
    gp.saved = c.at<float>(c.w.saved);
    if (d.det) gp.rowidx = c.at<int32_t>(c.w.iota), gp.dZ = c.at<float>(c.w.dx);     // (see det_scatter_kernel)
    gp.dh = c.at<float>(c.w.dhn);               // d loss / d h_n from the pooling backward, then d h_{t-1} step by step
    gp.state = c.at<float>(c.w.hn);             // (the pooling backward is done with h_n: d c / the GRU's direct term live there)
    const int H = d.H, GH = d.G * H, P = gp.P;
    const float *WcatT = c.at<const float>(c.w.WpT);
    float *gx = c.at<float>(c.w.gx);
    {
        StageTimer tm(c.ctx, ST_SEQ_BWD, c.stream);
        for (int t = d.L - 1; t >= 0; t--) {
            gp.t = t;
            if (int rc = launch_gen_cell_bwd(c.stream, gp)) return rc;
            // [dx_t | dh_{t-1}] = dG_t . [W_ih | W_hh]      (step 0: the dx half suffices)
            // (a forward through the transposed weights WcatT [2 H, G H])
            const GemmParams g = gemm_linear_fwd(gp.pre + (size_t)t * GH, (int64_t)d.L * GH, WcatT, GH, gx, 2 * H, P, GH,
                                                 t == 0 ? H : 2 * H);
            if (int rc = launch_gemm3(c.stream, gemm3_of(g))) return rc;
            if (int rc = launch_gen_scatter(c.stream, gp)) return rc;
        }
    }
    return PN_OK;
}

// true when max |Z| (SeqRange.x, the fp16 recurrence's operand range) is taken in the bank GEMM's epilogue: dense bank and
// fc0 both on gemm_kernel in this call -- fc0's launch clears the slot, the bank's adds to it, both on the caller's stream
// (range_rows_kernel and its place on the critical path between the bank and the recurrence are then not needed, and
// range_part_kernel on the packing stream must NOT clear the slot: it would race the bank)
inline bool bank_epilogue_range(const Call &c) {
    const Dims &d = c.d;
    const pn_pagg_args *a = c.a;
    return d.math == PN_SEQ_MATH_F16X2 && d.G > 0 && !d.generic && !d.compact && a->reuse_tables == 0 && !a->Xh_in &&
           !gemm3_pays(c.ctx, d.N, d.H, d.F, G3_FC0) && !gemm3_pays(c.ctx, d.N, d.L * d.H, d.H, G3_BANK);
}

int run_pack_fwd(const Call &c, hipStream_t s) {
    const Dims &d = c.d;
    if (d.G == 0) return PN_OK;         // mean / sum: nothing to pack
    if (d.generic)
        return launch_gen_pack(s, c.a->w_ih, c.a->w_hh, c.a->b_ih, c.a->b_hh, d.H, d.G, d.gru, c.at<float>(c.w.Wp),
                               c.at<float>(c.w.WpT), c.at<float>(c.w.biasc));
    if (d.math == PN_SEQ_MATH_F16X2) {      // two fp16 planes, scaled by the weights' own maxima (pn_seqh.hip)
        SeqRange *rg = c.at<SeqRange>(c.w.range);
        // (it also clears the slots this call's atomicMax launches add to; a reused dense bank keeps its range.x.)  A training
        // forward packs the BPTT's planes in the same launch, on the side stream under fc0 / the bank: the backward that follows
        // on this workspace then starts on its first real kernel (an inference forward uses that slot for Wcat)
        return launch_pack_fb(s, c.a->w_ih, c.a->w_hh, c.a->b_ih, c.a->b_hh, d.H, d.G, d.Gw, d.gru,
                              (d.compact || c.a->reuse_tables != 1) && !bank_epilogue_range(c), rg, c.at<void>(c.w.wmax),
                              c.at<void>(c.w.Wp), c.at<float>(c.w.biasc), c.a->no_save ? nullptr : c.at<void>(c.w.WpT));
    }
    return launch_pack_fwd3(s, c.a->w_ih, c.a->w_hh, c.a->b_ih, c.a->b_hh, d.H, d.G, d.gru, c.at<void>(c.w.Wp),
                            c.at<float>(c.w.biasc));
}

// the order-agnostic encoders (cell = mean / sum): forward or backward of micro-batch b
int run_seq_reduce(const Call &c, int b, bool backward) {
    const Dims &d = c.d;
    const pn_pagg_args *a = c.a;
    SeqReduceParams rp{};
    rp.Z = c.Z;
    rp.rowidx = c.at<int32_t>(c.w.rowidx);
    rp.slotof = c.at<int32_t>(c.w.slotof);
    rp.hn = c.at<float>(c.w.hn);
    rp.dhn = c.at<float>(c.w.dhn);
    rp.dZ = c.at<float>(c.w.dZ);
    rp.P = c.groups(b) * d.W;
    rp.L = d.L;
    rp.H = d.H;
    rp.Pmask = d.P_total;
    rp.scale = d.cell == CELL_MEAN ? 1.0f / (float)d.L : 1.0f;
    rp.p_drop = a->p_seq;
    rp.seed = a->seed;
    rp.dyn = a->step_state;
    rp.mask = a->mask_seq;
    if (backward && d.det) rp.rowidx = c.at<int32_t>(c.w.iota), rp.dZ = c.at<float>(c.w.dx);     // (see det_scatter_kernel)
    StageTimer tm(c.ctx, backward ? ST_SEQ_BWD : ST_SEQ_FWD, c.stream);
    return launch_seq_reduce(c.stream, rp, backward);
}

// Inference without dropout on the fp16 kernels: the input half of the gates is applied to the rows of the bank once
// (ZW = Z . W_ih^T + b, seq_fwdzw_kernel in pn_seqh.hip) when the table fits the slot the saved gates would take.
// PN_EVAL_ZW=0 switches it off (A/B runs, tests of the plain inference path).
inline bool use_zw(const Call &c) {
    const Dims &d = c.d;
    const pn_pagg_args *a = c.a;
    if (d.math != PN_SEQ_MATH_F16X2 || !a->no_save || a->p_seq > 0.0f || a->mask_seq) return false;
    if (knobs_of(c.ctx).eval_zw == 0) return false;
    const size_t need = (size_t)d.ZR * d.G * d.H * 4, have = (size_t)d.Sb * d.W * d.L * d.SV * d.H * 4;
    return need <= have && need <= ((size_t)2 << 30);
}

// bound of the factor the sequence dropout applies to a gathered row: 1 / (1 - p), or 16 for explicit masks (the contract
// of pn_pagg_shape.seq_math)
inline float seq_xmul(const pn_pagg_args *a) {
    return a->mask_seq ? 16.0f : a->p_seq > 0.0f ? 1.0f / (1.0f - a->p_seq) : 1.0f;
}

int run_seq_fwd(const Call &c, int b, bool save) {
    const Dims &d = c.d;
    const pn_pagg_args *a = c.a;
    if (d.G == 0) return run_seq_reduce(c, b, false);
    if (d.generic) return run_seq_fwd_generic(c, b, save);
    SeqFwdParams sp{};
    sp.Z = c.Z;
    sp.rowidx = c.at<int32_t>(c.w.rowidx);
    sp.slotof = c.at<int32_t>(c.w.slotof);
    sp.Wp = c.at<float>(c.w.Wp);
    sp.biasc = c.at<float>(c.w.biasc);
    sp.hn = c.at<float>(c.w.hn);
    sp.saved = save ? c.at<float>(c.w.saved) : nullptr;
    sp.xh = save ? c.at<float>(c.w.xh) : nullptr;
    sp.keep = (!save || a->mask_seq || !(a->p_seq > 0.0f)) ? nullptr : c.at<uint8_t>(c.w.keep);
    sp.P = c.groups(b) * d.W;
    sp.L = d.L;
    sp.Pmask = d.P_total;
    sp.p_drop = a->p_seq;
    sp.seed = a->seed;
    sp.dyn = a->step_state;
    sp.mask = a->mask_seq;
    StageTimer tm(c.ctx, ST_SEQ_FWD, c.stream);
    if (!save && use_zw(c)) {
        sp.range = c.at<SeqRange>(c.w.range);
        sp.ZW = c.at<const float>(c.w.saved);
        return launch_seq_fwdzw(c.ctx, c.stream, d.H, d.Gw, sp);
    }
    if (d.math == PN_SEQ_MATH_F16X2) {
        sp.range = c.at<SeqRange>(c.w.range);
        sp.xmul = seq_xmul(a);
        return launch_seq_fwdh(c.ctx, c.stream, d.H, d.Gw, sp);
    }
    return launch_seq_fwd3(c.ctx, c.stream, d.H, d.Gw, sp);
}

PoolParams pool_fwd_params(const Call &c, int b, float *out) {
    const Dims &d = c.d;
    const pn_pagg_args *a = c.a;
    const int homo = d.variant == PN_VARIANT_HOMO;
    PoolParams pp{};
    pp.variant = d.variant;
    pp.S = c.groups(b);
    pp.W = d.W;
    pp.H = d.H;
    pp.C = d.C;
    pp.N = d.N;
    pp.goff = c.group0(b);
    pp.hn = c.at<float>(c.w.hn);
    pp.ego_tab = homo ? c.Z : c.Xh;
    pp.egoidx = c.at<int32_t>(c.w.egoidx);
    pp.Xh = c.Xh;
    pp.sel = c.sel(b);
    pp.att_w = a->att_w;
    pp.att_b = a->att_b;
    pp.fc2_w = a->fc2_w;
    pp.fc2_b = a->fc2_b;
    pp.p_drop = a->p_cls;
    pp.seed = a->seed;
    pp.dyn = a->step_state;
    pp.mask = a->mask_cls;
    pp.coef = c.at<float>(c.w.coef);
    pp.rawsc = c.at<float>(c.w.rawsc);
    pp.layer1 = c.at<float>(c.w.layer1);
    pp.out = out;
    pp.omega = c.omega;       // (laid out like ids without the last axis: the plan's slot q, less the slice's first)
    pp.slotof = c.at<int32_t>(c.w.slotof);
    pp.wbase = a->index_rows_local ? (int64_t)d.group_begin * d.W : 0;
    pp.norm = c.norm;
    return pp;
}
// outputs: pn_pagg_forward's own pass writes the caller's optional outputs (out_*: rows of micro-batch b); the backward's
// re-runs do not
int run_pool_fwd(const Call &c, int b, float *out, bool outputs = false) {
    PoolParams pp = pool_fwd_params(c, b, out);
    if (outputs) {
        const pn_pagg_args *a = c.a;
        const int64_t r0 = (int64_t)b * c.d.Sb;       // first row of the slice's outputs (= c.group0(b) - group_begin)
        if (a->out_embed) pp.embed = a->out_embed + r0 * 2 * c.d.H;
        if (a->out_path_weight) pp.path_weight = a->out_path_weight + r0 * c.d.W;
        if (a->out_path_state) pp.path_state = a->out_path_state + r0 * c.d.W * c.d.H;
    }
    StageTimer tm(c.ctx, ST_POOL_FWD, c.stream);
    return launch_pool_fwd(c.stream, pp);
}

int check_forward_args(const Call &c, const char *who) {
    const pn_pagg_args *a = c.a;
    const Dims &d = c.d;
    if (!a->ids || !a->codes || !a->sel || !a->bank_w || !a->bank_b || !a->fc2_w || !a->fc2_b || !a->out)
        PN_FAIL(PN_ERR_ARG, "%s: null tensor", who);
    if (d.G > 0 && (!a->w_ih || !a->w_hh || !a->b_ih || !a->b_hh)) PN_FAIL(PN_ERR_ARG, "%s: recurrent weights missing", who);
    if (!a->Xh_in && !a->reuse_tables && (!a->X || !a->fc0_w || !a->fc0_b)) PN_FAIL(PN_ERR_ARG, "%s: X / fc0 missing", who);
    if (d.variant != PN_VARIANT_PAGG && (!a->att_w || !a->att_b)) PN_FAIL(PN_ERR_ARG, "%s: attention weights missing", who);
    if (reinterpret_cast<uintptr_t>(a->out_path_state) % 16 != 0)
        PN_FAIL(PN_ERR_ARG, "%s: out_path_state must be 16-byte aligned", who);
    return PN_OK;
}

// What a forward does before its first micro-batch: the touched rows, the index plan of micro-batch 0 and the packed
// weights (second stream), Xh = fc0(X), Z = bank(Xh); joined, so that the recurrence can follow.
// zero_fill: flushed on the second stream behind the packing (pn_pagg_train_step: the zero fill of the backward's accumulators)
int run_tables(const Call &c, JoinGuard &joiner, ZeroFill *zero_fill = nullptr) {
    pn_context *ctx = c.ctx;
    hipStream_t stream = c.stream;
    const pn_pagg_args *a = c.a;
    const Dims &d = c.d;
    const int H = d.H, L = d.L;
    const int homo = d.variant == PN_VARIANT_HOMO;
    const bool epi_range = bank_epilogue_range(c);
    // the index plan (of the first micro-batch) and the weight packing do not depend on fc0 / bank: second stream,
    // joined before the recurrence
    if (d.compact) {        // the compact rows first: the index plan and the bank both read them
        // (they read ids / codes on `stream`, ahead of the fork: a walk enqueued on the second stream -- where
        //  pn_pagg_paths_stream places it -- is waited for first; the dense call reads them behind the fork only)
        if (int rc = context_wait_side(ctx, stream)) return rc;
        StageTimer tm(ctx, ST_PLAN_PACK, stream);
        if (int rc = run_compact_rows(c, stream)) return rc;
    }
    hipStream_t pstream = stream;
    if (!profiling_every_stage(ctx))
        if (void *side = context_fork(ctx, stream)) pstream = (hipStream_t)side;
    {
        StageTimer tm(ctx, ST_PLAN_PACK, pstream);
        if (int rc = run_plan(c, pstream, 0)) return rc;
        if (int rc = run_pack_fwd(c, pstream)) return rc;
    }
    if (zero_fill)
        if (int rc = zero_fill->flush(pstream)) return rc;
    if (pstream != stream)
        if (int rc = joiner.mark()) return rc;
    if (!a->reuse_tables) {
        // fc0 (+ReLU for HOMO): Xh = X . fc0_w^T + fc0_b
        if (!a->Xh_in) {
            StageTimer tm(ctx, ST_FC0, stream);
            GemmParams g = gemm_linear_fwd(a->X, d.F, a->fc0_w, d.F, c.at<float>(c.w.Xh), H, d.N, d.F, H);
            g.bias = a->fc0_b;
            g.relu = homo;
            g.clear_word = epi_range ? &c.at<SeqRange>(c.w.range)->x : nullptr;     // (epi_range: never with gemm3)
            if (c.sp) {         // prepared features: the non-zeros of a row against rows of fc0_w^T, same epilogue
                float *W0T = c.at<float>(c.w.w0t);
                if (int rc = launch_transpose(stream, a->fc0_w, H, d.F, W0T)) return rc;
                if (int rc = launch_sparse_fc0_fwd(stream, *c.sp, d.N, H, W0T, g.bias, g.relu, g.clear_word, g.C)) return rc;
            } else if (gemm3_pays(c.ctx, d.N, H, d.F, G3_FC0)) {          // large graphs: fp32 results from the bf16 matrix pipe (six MFMAs per product)
                if (int rc = launch_gemm3(stream, gemm3_of(g))) return rc;
            } else if (int rc = launch_gemm_split(stream, g, c.at<float>(c.w.gpart)))
                return rc;
        }
    }
    // node-sharded path: the caller's all-gather of Xh runs on its own stream; this one waits for it here, where Xh is first
    // read -- everything above (touched rows, plan, packing) has been enqueued under it
    if (a->Xh_in && a->Xh_ready) PN_CHECK_HIP(hipStreamWaitEvent(stream, (hipEvent_t)a->Xh_ready, 0));
    if (d.compact) {
        // distance bank over the touched rows: code by code, Z[compact row] = act(Xh[node] . bank_w[code]^T + bank_b[code])
        // (the touched set belongs to this batch: reuse_tables keeps the projected features only)
        StageTimer tm(ctx, ST_BANK, stream);
        const int mmax = (int)std::min<int64_t>(d.N, d.ZR);
        for (int code = 0; code < L; code++) {
            GemmParams g = gemm_linear_fwd(c.Xh, H, a->bank_w + (size_t)code * H * H, H, c.Z, H, mmax, H, H);
            g.bias = a->bank_b + (size_t)code * H;
            g.relu = homo;
            g.ind = GEMM_IND_A_ROWS;
            g.seg = c.at<const int32_t>(c.w.seg) + code;
            g.list = c.at<const int32_t>(c.w.list);
            if (gemm3_pays(c.ctx, mmax, H, H, G3_BANK)) {
                if (int rc = launch_gemm3(stream, gemm3_of(g), g.ind)) return rc;
            } else if (int rc = launch_gemm(stream, g))
                return rc;
        }
    } else if (a->reuse_tables != 1) {      // (1: the dense Z of the previous forward is still valid; 2: only Xh is)
        // distance bank over every node: Z[v, d, :] = act(Xh[v] . bank_w[d]^T + bank_b[d])
        StageTimer tm(ctx, ST_BANK, stream);
        GemmParams g = gemm_linear_fwd(c.Xh, H, a->bank_w, H, c.Z, (int64_t)L * H, d.N, H, L * H);
        g.bias = a->bank_b;
        g.relu = homo;
        g.absmax = epi_range ? &c.at<SeqRange>(c.w.range)->x : nullptr;         // (epi_range: never with gemm3)
        if (gemm3_pays(c.ctx, d.N, L * H, H, G3_BANK)) {
            if (int rc = launch_gemm3(stream, gemm3_of(g))) return rc;
        } else if (int rc = launch_gemm(stream, g))
            return rc;
    }
    // the fp16 recurrence scales the gathered rows by a power of two taken from the largest |Z| of the rows just computed
    // (a reused dense Z keeps its record: it sits next to Z in the workspace)
    if (int rc = joiner.join()) return rc;      // the recurrence needs the plan and the packed weights
    // (after the join: the packing stream's range_part_kernel cleared the slot this launch adds to)
    if (d.math == PN_SEQ_MATH_F16X2 && (d.compact || a->reuse_tables != 1) && !epi_range) {
        StageTimer tm(ctx, ST_BANK, stream);
        if (int rc = launch_range_rows(stream, c.Z, d.ZR, H, d.compact ? c.at<const int32_t>(c.w.seg) + L : nullptr,
                                       c.at<SeqRange>(c.w.range)))
            return rc;
    }
    if (use_zw(c)) {
        // ZW [rows of Z, G*H] = Z . W_ih^T + (b_ih + b_hh)  (GRU: its four slots): Wcat in the slot of the backward's packed
        // weights, the table in the slot of the saved gates -- neither is used by an inference forward
        StageTimer tm(ctx, ST_BANK, stream);
        const int GH = d.G * H;
        float *Wcat = c.at<float>(c.w.WpT);
        if (int rc = launch_gen_pack(stream, a->w_ih, a->w_hh, a->b_ih, a->b_hh, H, d.G, d.gru, Wcat, nullptr, c.at<float>(c.w.biasc)))
            return rc;
        const int M = (int)d.ZR;
        const bool g3 = H % G3_KT == 0 && (int64_t)((M + G3_BM - 1) / G3_BM) * ((GH + G3_BN - 1) / G3_BN) >= 256;
        GemmParams g = gemm_linear_fwd(c.Z, H, Wcat, 2 * H, c.at<float>(c.w.saved), GH, M, H, GH);
        g.bias = c.at<float>(c.w.biasc);
        if (g3) {
            if (int rc = launch_gemm3(stream, gemm3_of(g))) return rc;
        } else if (int rc = launch_gemm(stream, g))
            return rc;
    }
    return PN_OK;
}

// ---- deterministic mode: the three scatters of a backward and their destination orders ------------------------------------
// dst[key[i]] += contribution i, added in the order of i, for  DET_SEL  the ego half of d layer1 onto the masked nodes' rows
// of d Xh (keys: sel),  DET_EGO  the attention-ego term onto the ego rows (keys: egoidx),  DET_ROW  the gather backward
// (keys: rowidx).  All three key arrays come out of the index plan -- nothing of the backward enters them -- so their
// stable sort by key runs ONCE per micro-batch, right behind the plan and on the context's second stream under the
// forward's recurrence (round 5; until then: a radix sort in front of each scatter, on the backward's critical path --
// 0.10 of the 0.27 ms the mode cost at the headline shape were the pooling backward's two sorts alone).
enum { DET_SEL = 0, DET_EGO = 1, DET_ROW = 2 };
struct DetOrder {
    const int32_t *keys;
    int64_t K, max_key;
};
inline DetOrder det_order(const Call &c, int which, int b) {
    const Dims &d = c.d;
    const int64_t Sb = c.groups(b), Pb = Sb * d.W;
    const bool homo = d.variant == PN_VARIANT_HOMO;
    switch (which) {
        case DET_SEL: return DetOrder{c.sel(b), Sb, (int64_t)d.N - 1};
        case DET_EGO: return DetOrder{c.at<const int32_t>(c.w.egoidx), Pb, homo ? d.ZR - 1 : (int64_t)d.N - 1};
        default: return DetOrder{c.at<const int32_t>(c.w.rowidx), Pb * d.L, d.ZR - 1};
    }
}

// the one sort's three segments for micro-batch b: their keys, lengths (EGO is empty without attention), offsets in the sorted
// output (the running sum of the lengths), the largest key of a present segment and the bits it takes
struct DetSegments {
    DetOrder o[3];
    int64_t n[3], off[3], total, max_key;
    int bits;
};
DetSegments det_segments(const Call &c, int b) {
    const bool has_att = c.d.variant != PN_VARIANT_PAGG;
    DetSegments g{};
    for (int which = 0; which < 3; which++) {
        g.o[which] = det_order(c, which, b);
        g.n[which] = (which == DET_EGO && !has_att) ? 0 : std::max<int64_t>(g.o[which].K, 0);
        g.off[which] = g.total;
        g.total += g.n[which];
        if (g.n[which]) g.max_key = std::max(g.max_key, g.o[which].max_key);
    }
    g.bits = 1;
    while (g.bits < 31 && (g.max_key >> g.bits) != 0) g.bits++;
    return g;
}

int prepare_det_orders(const Call &c, hipStream_t s, int b) {
    const DetSegments g = det_segments(c, b);
    if (g.total <= 0) return PN_OK;
    if (g.bits + 2 > 31)
        PN_FAIL(PN_ERR_ARG, "deterministic mode: %lld table rows leave no room for the scatters' segment bits", (long long)g.max_key + 1);
    DetKeys3 q{};
    for (int which = 0; which < 3; which++) {
        q.keys[which] = g.o[which].keys;
        q.n[which] = g.n[which];
        q.hi[which] = (int32_t)g.o[which].max_key;
    }
    q.shift = g.bits;
    int32_t *ck = c.at<int32_t>(c.w.keys), *pos = c.at<int32_t>(c.w.skey);
    if (int rc = launch_det_keys3(s, q, g.total, ck, pos)) return rc;
    // (okey / osrc are the heads of the two contiguous output blocks; an empty EGO segment leaves its slot unused: the
    //  segments that follow start where the sort puts them only if the layout matches -- so the outputs are addressed by the
    //  running sum of the ACTUAL counts, which equals the layout's whenever a segment is present)
    return sort_pairs_i32(c.at<void>(c.w.stmp), c.w.stmp_bytes, ck, c.at<int32_t>(c.w.okey), pos, c.at<int32_t>(c.w.osrc),
                          g.total, g.bits + 2, s);
}

// the orders of micro-batch b on the second stream when there is one (joined by the guard on the way out), else in line
int fork_det_orders(const Call &c, JoinGuard &joiner, int b) {
    hipStream_t s = c.stream;
    if (!profiling_every_stage(c.ctx))
        if (void *side = context_fork(c.ctx, c.stream)) s = (hipStream_t)side;
    if (int rc = prepare_det_orders(c, s, b)) return rc;
    if (s != c.stream) return joiner.mark();
    return PN_OK;
}

// where the one sort left scatter `which` of micro-batch b
DetScatterParams det_params(const Call &c, int which, int b, const float *rows, const float *scal, const float *vec, float *dst) {
    const DetSegments g = det_segments(c, b);
    const int64_t off = g.off[which];
    return DetScatterParams{c.at<int32_t>(c.w.okey) + off, c.at<int32_t>(c.w.osrc) + off, (int32_t)((1u << g.bits) - 1u),
                            g.n[which], off / DET_CHUNK + which, rows, scal, vec, dst, c.at<float>(c.w.cpart), c.d.H};
}

int run_det_scatter(const Call &c, int which, int b, const float *rows, const float *scal, const float *vec, float *dst) {
    const DetScatterParams p = det_params(c, which, b, rows, scal, vec, dst);
    return launch_det_scatters(c.stream, &p, 1);
}

// ---- the backward's stages (pagg_backward_impl) ---------------------------------------------------------------------------
// d Xh: the caller's g_Xh in a node-sharded call (Xh_in), else the workspace's
inline float *grad_xh(const Call &c) { return c.a->Xh_in ? c.a->g_Xh : c.at<float>(c.w.dXh); }

// the context's second stream, forked from the call's, when `fork` and there is one -- else the call's stream
inline hipStream_t fork_if(const Call &c, bool fork) {
    if (fork)
        if (void *side = context_fork(c.ctx, c.stream)) return (hipStream_t)side;
    return c.stream;
}

// classifier of micro-batch b on `s`: g_fc2_w += g_out^T . layer1, g_fc2_b += colsum(g_out) -- nothing later reads them.
// loss (behind the fused pooling step): first the fixed-order sum of the per-node loss terms into loss[0].
// On the second stream the end is marked for the join.
int run_fc2_grad(const Call &c, int b, JoinGuard &joiner, hipStream_t s, const float *g_out, float *loss, float grad_scale,
                 const LossOpts *opts) {
    const Dims &d = c.d;
    const pn_pagg_args *a = c.a;
    const int H = d.H, Sb = c.groups(b);
    if (loss)
        if (int rc = launch_loss_sum(s, c.at<const float>(c.w.outb), Sb, grad_scale, opts, loss, d.nb == 1)) return rc;
    if (g_out) {        // (no g_out: only the embedding is differentiated, g_fc2_* keep the backward's zero fill)
        StageTimer tm(c.ctx, ST_FC2_GRAD, s);
        GemmParams g = gemm_weight_grad(g_out, d.C, c.at<float>(c.w.layer1), 2 * H, a->g_fc2_w, 2 * H, Sb, 2 * H, d.C);
        g.rowsum = a->g_fc2_b;          // g_fc2_b = row sums of the A operand (g_out^T)
        g.mode = GEMM_ATOMIC;
        if (a->g_fc2_w && d.det) {
            if (int rc = launch_gemm_det(s, g, (Sb + 127) / 128, c.at<float>(c.w.dgemm))) return rc;
        } else if (a->g_fc2_w) {
            if (int rc = launch_gemm(s, g, (Sb + 127) / 128)) return rc;
        } else if (a->g_fc2_b) {
            if (int rc = launch_colsum(s, g_out, nullptr, d.C, Sb, d.C, a->g_fc2_b, d.det)) return rc;
        }
    }
    return s != c.stream ? joiner.mark() : PN_OK;
}

// pooling / attention backward of micro-batch b -> dhn, dXh (ego rows), dZ or dXh (attention ego), g_att_*
PoolBwdParams pool_bwd_params(const Call &c, int b, const float *g_out) {
    const Dims &d = c.d;
    const pn_pagg_args *a = c.a;
    const int homo = d.variant == PN_VARIANT_HOMO;
    float *dXh = grad_xh(c), *scratch = c.at<float>(c.w.dl1);
    PoolBwdParams pp{};
    pp.variant = d.variant;
    pp.S = c.groups(b);
    pp.W = d.W;
    pp.H = d.H;
    pp.C = d.C;
    pp.N = d.N;
    pp.goff = c.group0(b);
    pp.hn = c.at<float>(c.w.hn);
    pp.ego_tab = homo ? c.Z : c.Xh;
    pp.egoidx = c.at<int32_t>(c.w.egoidx);
    pp.sel = c.sel(b);
    pp.att_w = a->att_w;
    pp.fc2_w = a->fc2_w;
    pp.g_out = g_out;
    pp.coef = c.at<float>(c.w.coef);
    pp.rawsc = c.at<float>(c.w.rawsc);
    pp.p_drop = a->p_cls;
    pp.seed = a->seed;
    pp.dyn = a->step_state;
    pp.mask = a->mask_cls;
    pp.dhn = c.at<float>(c.w.dhn);
    pp.dXh = dXh;
    pp.dego = homo ? c.at<float>(c.w.dZ) : dXh;
    // attention gradients are optional outputs: fall back to scratch so the kernel needs no branches
    pp.g_att_w = a->g_att_w ? a->g_att_w : scratch;
    pp.g_att_b = a->g_att_b ? a->g_att_b : scratch + 2 * d.H;
    // the attention-weight terms always go through per-workgroup partials + an ordered reduce: 325 workgroups adding
    // to the same 2H + 1 addresses with atomics serialise
    pp.det_att = c.at<float>(c.w.datt);
    if (d.det) {
        pp.det_sel = c.at<float>(c.w.dsel);
        pp.det_ds = c.at<float>(c.w.dds);
    }
    pp.omega = c.omega;
    pp.slotof = c.at<int32_t>(c.w.slotof);
    pp.wbase = a->index_rows_local ? (int64_t)d.group_begin * d.W : 0;
    pp.norm = c.norm;
    return pp;
}

// pn_pagg_train_step, default mode: pooling forward, loss and pooling backward of micro-batch b in one launch (which kernel:
// launch_pool_step, pn_pool.hip)
int run_pool_step(const Call &c, int b, const PoolBwdParams &pp, const int64_t *target, float grad_scale, const LossOpts *opts) {
    const Dims &d = c.d;
    PoolStepParams ps{};
    ps.f = pool_fwd_params(c, b, c.a->out + (size_t)b * d.Sb * d.C);
    ps.b = pp;
    ps.target = target + (size_t)b * d.Sb;
    ps.scale = grad_scale;
    ps.gout = c.at<float>(c.w.gout);
    ps.b.g_out = ps.gout;
    ps.lossg = c.at<float>(c.w.outb);       // (the fused step's logits go to the caller: the slot is free)
    StageTimer tm(c.ctx, ST_POOL_FWD, c.stream);
    return launch_pool_step(c.ctx, c.stream, ps, opts, knobs_of(c.ctx).pool_step);
}

// the pooling backward (pool_bwd_wg_kernel) in its stage bracket -- an empty bracket behind the pooling step, which did it
int run_pool_bwd(const Call &c, const PoolBwdParams &pp, bool pool_step) {
    StageTimer tm(c.ctx, ST_POOL_BWD, c.stream);
    if (pool_step) return PN_OK;
    return launch_pool_bwd(c.ctx, c.stream, pp);
}

// the attention weights' terms in workgroup order (a partial per workgroup of the pooling backward) on `s`; on the second
// stream the end is marked for the join
int run_att_reduce(const Call &c, JoinGuard &joiner, hipStream_t s, const PoolBwdParams &pp) {
    if (c.d.variant != PN_VARIANT_PAGG)
        if (int rc = launch_att_reduce(s, pp.det_att, pp.S, pp.H, pp.g_att_w, pp.g_att_b)) return rc;
    return s != c.stream ? joiner.mark() : PN_OK;
}

// deterministic mode: the ego half of d layer1 onto the masked nodes' rows of dXh; the attention-ego term onto the ego rows
// (one launch per pass for the two: they write different rows -- or, for the hetero / PAGG classes whose ego rows live in
//  dXh as well, the same rows in a fixed order: SEL, then EGO in launches of its own)
int run_pool_scatters(const Call &c, int b, const PoolBwdParams &pp) {
    const bool has_att = c.d.variant != PN_VARIANT_PAGG;
    const DetScatterParams two[2] = {det_params(c, DET_SEL, b, pp.det_sel, nullptr, nullptr, pp.dXh),
                                     det_params(c, DET_EGO, b, nullptr, pp.det_ds, c.a->att_w + c.d.H, pp.dego)};
    if (has_att && pp.dego != pp.dXh) return launch_det_scatters(c.stream, two, 2);
    if (int rc = launch_det_scatters(c.stream, two, 1)) return rc;
    return has_att ? launch_det_scatters(c.stream, two + 1, 1) : PN_OK;
}

// BPTT of micro-batch b and the gather-backward scatter (mean / sum encoders: the scatter alone) -- run_seq_fwd's counterpart
int run_seq_bwd(const Call &c, int b) {
    const Dims &d = c.d;
    const pn_pagg_args *a = c.a;
    const bool f16 = d.math == PN_SEQ_MATH_F16X2;
    const int64_t Pb = (int64_t)c.groups(b) * d.W;
    float *dZ = c.at<float>(c.w.dZ);
    // (deterministic mode: the fp16 BPTT stores its dx rows outright; the other kernels add into a zero-filled buffer)
    if (d.det && !f16) PN_CHECK_HIP(hipMemsetAsync(c.at<float>(c.w.dx), 0, (size_t)Pb * d.L * d.H * sizeof(float), c.stream));
    if (d.G == 0) {
        if (int rc = run_seq_reduce(c, b, true)) return rc;
    } else if (d.generic) {
        if (int rc = run_seq_bwd_generic(c, b)) return rc;
    } else {
        StageTimer tm(c.ctx, ST_SEQ_BWD, c.stream);
        SeqBwdParams sp{};
        sp.saved = c.at<float>(c.w.saved);
        sp.keep = (a->mask_seq || !(a->p_seq > 0.0f)) ? nullptr : c.at<const uint8_t>(c.w.keep);
        sp.dhn = c.at<float>(c.w.dhn);
        sp.rowidx = c.at<int32_t>(c.w.rowidx);
        sp.slotof = c.at<int32_t>(c.w.slotof);
        sp.WpT = c.at<float>(c.w.WpT);
        sp.dG = c.at<float>(c.w.dG);
        sp.dZ = dZ;
        sp.P = (int)Pb;
        sp.L = d.L;
        sp.Pmask = d.P_total;
        sp.p_drop = a->p_seq;
        sp.seed = a->seed;
        sp.mask = a->mask_seq;
        sp.merge0 = d.variant != PN_VARIANT_HETERO && !d.det;   // (the hetero plan's step-0 rows are other paths' far ends: no runs)
        if (d.det) sp.rowidx = c.at<int32_t>(c.w.iota), sp.dZ = c.at<float>(c.w.dx);     // (see det_scatter_kernel)
        sp.range = c.at<SeqRange>(c.w.range);
        sp.store_dx = d.det && f16;
        if (int rc = f16 ? launch_seq_bwdh(c.ctx, c.stream, d.H, d.Gw, sp) : launch_seq_bwd3(c.ctx, c.stream, d.H, d.Gw, sp))
            return rc;
    }
    if (d.det) {        // the stored mask * dx rows onto their table rows, in the order of the path steps
        StageTimer tm(c.ctx, ST_SEQ_BWD, c.stream);
        return run_det_scatter(c, DET_ROW, b, c.at<float>(c.w.dx), nullptr, nullptr, dZ);
    }
    return PN_OK;
}

// recurrent weight / bias gradients: [g_W_ih | g_W_hh] (+)= dG^T . XH, g_b (+)= colsum(dG) over the Pb * L rows of micro-batch
// b: K-split partials into `wpart`, then their reduction.  Second stream (also in deterministic mode: the partials are
// reduced in a fixed order, streams do not reorder a kernel's sums); the call's stream waits for it on the way out.
int run_wgrad(const Call &c, int b, JoinGuard &joiner) {
    const Dims &d = c.d;
    const pn_pagg_args *a = c.a;
    const int H = d.H, GH = d.G * H;
    const hipStream_t ws = fork_if(c, !profiling_every_stage(c.ctx));
    WgradParams wp{};
    wp.dG = c.at<float>(c.w.dG);
    wp.xh = c.at<const float>(c.w.xh);
    wp.R = (int64_t)c.groups(b) * d.W * d.L;
    wp.GH = GH;
    wp.H2 = 2 * H;
    int nz = c.w.wgrad_split;
    // a node-sharded caller runs its reduce-scatter of d Xh (RCCL's kernels) and fc0's backward under this launch
    // (g_Xh_ready): they need CUs whose registers are not all taken, whatever the launch's length
    if (a->Xh_in && a->g_Xh_ready) nz = std::min(nz, std::max(1, (WGRAD_CUS_SHARED + c.w.wgrad_tiles - 1) / c.w.wgrad_tiles));
    int64_t rps = (wp.R + nz - 1) / nz;
    rps = (rps + WG_KT - 1) / WG_KT * WG_KT;
    wp.rows_per_split = rps;
    const int64_t ntiles = (wp.R + WG_KT - 1) / WG_KT;
    const int nz_used = (int)(ntiles < nz ? ntiles : nz);
    wp.part_w = c.at<float>(c.w.wpart);
    wp.part_b = wp.part_w + (size_t)nz * GH * 2 * H;
    {
        StageTimer tm(c.ctx, ST_WGRAD, ws);
        int nz_red = nz_used;
        wp.range = c.at<SeqRange>(c.w.range);
        wp.xmul = seq_xmul(a);
        if (d.math == PN_SEQ_MATH_F16X2) {      // the two-stage pipeline on fp16 planes (pn_seqh.hip)
            const int64_t nt16 = (wp.R + 15) / 16;
            nz_red = (int)(nt16 < nz ? nt16 : nz);
            if (int rc = launch_wgradh(c.ctx, ws, wp, H, nz_red)) return rc;
        } else if (seq4_select(c.ctx, H, d.G, d.L) & SEQ4_WGRAD) {     // two-stage pipeline over K tiles of 16 rows (pn_seq4.hip)
            const int64_t nt16 = (wp.R + 15) / 16;
            nz_red = (int)(nt16 < nz ? nt16 : nz);
            if (int rc = launch_wgrad4(c.ctx, ws, wp, nz_red)) return rc;
        } else {
            if (int rc = launch_wgrad3(c.ctx, ws, wp, nz_used)) return rc;
        }
        if (int rc = launch_wgrad_reduce(ws, wp.part_w, wp.part_b, nz_red, GH, H, b > 0 ? 1 : 0, d.gru,
                                         a->g_w_ih, a->g_w_hh, a->g_b_ih, a->g_b_hh))
            return rc;
    }
    return ws != c.stream ? joiner.mark() : PN_OK;
}

// distance bank backward (ReLU gate for HOMO): dXh += dZ' . bank_w ; g_bank_w = dZ'^T . Xh.  First every code's
// contribution to d Xh (what a sharded caller's reduce-scatter waits for: g_Xh_ready), then the weight gradients.
int run_bank_bwd(const Call &c, float *dXh, const float *dZ) {
    pn_context *ctx = c.ctx;
    hipStream_t stream = c.stream;
    const pn_pagg_args *a = c.a;
    const Dims &d = c.d;
    const int H = d.H, L = d.L;
    const float *Xh = c.Xh, *zgate = d.variant == PN_VARIANT_HOMO ? c.Z : nullptr;
    float *dgemm = d.det ? c.at<float>(c.w.dgemm) : nullptr;
    StageTimer tm(ctx, ST_BANK_BWD, stream);
    if (d.compact) {
        // over the touched rows, code by code (the compact rows of a code are distinct nodes: += without atomics):
        //   dXh[node] += dZ'[row] . bank_w[code],   g_bank_w[code] += dZ'[rows]^T . Xh[nodes],   g_bank_b[code] += colsum
        if (a->g_bank_b && !a->g_bank_w) PN_FAIL(PN_ERR_ARG, "pn_pagg_backward: compact rows need g_bank_w with g_bank_b");
        const int mmax = (int)std::min<int64_t>(d.N, d.ZR);
        const int32_t *seg = c.at<const int32_t>(c.w.seg), *list = c.at<const int32_t>(c.w.list);
        // (the 64 x 64 kernel: at the 10 M-node shape the 128 x 128 tiles' read-modify-write of scattered dXh rows at two
        //  workgroups per CU measured slower, 24.1 vs 21.6 ms for the stage)
        for (int code = 0; code < L; code++) {
            GemmParams g = gemm_input_grad(dZ, H, a->bank_w + (size_t)code * H * H, H, dXh, H, mmax, H, H);
            g.gateA = zgate;
            g.mode = GEMM_ADD;
            g.ind = GEMM_IND_C_ROWS;
            g.seg = seg + code;
            g.list = list;
            if (int rc = launch_gemm(stream, g)) return rc;
        }
        if (a->Xh_in && a->g_Xh_ready) PN_CHECK_HIP(hipEventRecord((hipEvent_t)a->g_Xh_ready, stream));
        for (int code = 0; code < L; code++) {
            GemmParams g = gemm_weight_grad(dZ, H, Xh, H, a->g_bank_w ? a->g_bank_w + (size_t)code * H * H : nullptr, H, mmax, H, H);
            g.gateA = zgate;
            g.rowsum = a->g_bank_b ? a->g_bank_b + (size_t)code * H : nullptr;
            g.mode = GEMM_ATOMIC;
            g.ind = GEMM_IND_K;
            g.seg = seg + code;
            g.list = list;
            if (a->g_bank_w && d.det) {
                if (int rc = launch_gemm_det(stream, g, (mmax + 255) / 256, dgemm)) return rc;
            } else if (a->g_bank_w && rgrad_pays(ctx, mmax, H, H)) {         // large graphs: the bf16 x 3 row-reduction kernel
                const RgradParams rp{dZ, zgate, Xh, H, H, mmax, H, H, a->g_bank_w + (size_t)code * H * H, H,
                                     a->g_bank_b ? a->g_bank_b + (size_t)code * H : nullptr, seg + code, list};
                if (int rc = launch_rgrad(ctx, stream, rp)) return rc;
            } else if (a->g_bank_w)
                if (int rc = launch_gemm(stream, g, (mmax + 255) / 256)) return rc;
        }
        return PN_OK;
    }
    if (gemm3_pays(ctx, d.N, H, L * H, G3_BANK_DX)) {        // bank_w [L*H, H] -> [H, L*H]
        float *bankT = c.at<float>(c.w.bankT);
        launch_transpose(stream, a->bank_w, L * H, H, bankT);
        GemmParams g = gemm_linear_fwd(dZ, (int64_t)L * H, bankT, (int64_t)L * H, dXh, H, d.N, L * H, H);
        g.gateA = zgate;
        g.mode = GEMM_ADD;
        if (int rc = launch_gemm3(stream, gemm3_of(g))) return rc;
    } else {
        GemmParams g = gemm_input_grad(dZ, (int64_t)L * H, a->bank_w, H, dXh, H, d.N, H, L * H);
        g.gateA = zgate;
        g.mode = GEMM_ADD;
        if (int rc = launch_gemm_split(stream, g, c.at<float>(c.w.gpart))) return rc;
    }
    if (a->Xh_in && a->g_Xh_ready) PN_CHECK_HIP(hipEventRecord((hipEvent_t)a->g_Xh_ready, stream));
    GemmParams g = gemm_weight_grad(dZ, (int64_t)L * H, Xh, H, a->g_bank_w, H, d.N, H, L * H);
    g.gateA = zgate;
    g.rowsum = a->g_bank_b;         // g_bank_b rides along as the row sums of the same (gated) A operand
    g.mode = GEMM_ATOMIC;
    if (a->g_bank_w && d.det) {
        if (int rc = launch_gemm_det(stream, g, (d.N + 255) / 256, dgemm)) return rc;
    } else if (a->g_bank_w && rgrad_pays(ctx, d.N, L * H, H)) {
        const RgradParams rp{dZ, zgate, Xh, (int64_t)L * H, H, d.N, L * H, H, a->g_bank_w, H, a->g_bank_b, nullptr, nullptr};
        if (int rc = launch_rgrad(ctx, stream, rp)) return rc;
    } else if (a->g_bank_w) {
        if (int rc = launch_gemm(stream, g, (d.N + 255) / 256)) return rc;
    } else if (a->g_bank_b) {
        if (int rc = launch_colsum(stream, dZ, zgate, (int64_t)L * H, d.N, L * H, a->g_bank_b, d.det)) return rc;
    }
    return PN_OK;
}

// fc0 backward (ReLU gate for HOMO): g_fc0_w / g_fc0_b from dXh and X, then g_X = dXh' . fc0_w
int run_fc0_bwd(const Call &c, const float *dXh) {
    pn_context *ctx = c.ctx;
    hipStream_t stream = c.stream;
    const pn_pagg_args *a = c.a;
    const Dims &d = c.d;
    const int H = d.H;
    const float *xgate = d.variant == PN_VARIANT_HOMO ? c.Xh : nullptr;
    StageTimer tm(ctx, ST_FC0_BWD, stream);
    GemmParams g = gemm_weight_grad(dXh, H, a->X, d.F, a->g_fc0_w, d.F, d.N, d.F, H);
    g.gateA = xgate;
    g.rowsum = a->g_fc0_b;
    g.mode = GEMM_ATOMIC;
    if (a->g_fc0_w && c.sp) {       // prepared features: a column's entries in a fixed order (deterministic mode included)
        // (the bias gradient rides along as extra workgroups of the launch; fixed-order mode: the one-add-per-output column sum)
        if (int rc = launch_sparse_fc0_wgrad(stream, *c.sp, d.N, d.F, H, dXh, xgate, a->g_fc0_w, d.det ? nullptr : a->g_fc0_b)) return rc;
        if (a->g_fc0_b && d.det)
            if (int rc = launch_colsum(stream, dXh, xgate, H, d.N, H, a->g_fc0_b, true)) return rc;
    } else if (a->g_fc0_w && d.det) {
        if (int rc = launch_gemm_det(stream, g, (d.N + 255) / 256, c.at<float>(c.w.dgemm))) return rc;
    } else if (a->g_fc0_w && d.F % 4 == 0 && rgrad_pays(ctx, d.N, H, d.F)) {
        const RgradParams rp{dXh, xgate, a->X, H, d.F, d.N, H, d.F, a->g_fc0_w, d.F, a->g_fc0_b, nullptr, nullptr};
        if (int rc = launch_rgrad(ctx, stream, rp)) return rc;
    } else if (a->g_fc0_w && xpad_floats(d) > 0 && rgrad_pays(ctx, d.N, H, (d.F + 3) / 4 * 4)) {
        // rows of X padded to 16 bytes first (see xpad_floats); the padding columns are zeros, and outputs past F are not stored
        const int F4 = (d.F + 3) / 4 * 4;
        float *Xp = c.at<float>(c.w.xpad);
        if (int rc = launch_pad_rows(stream, a->X, (int64_t)d.N, d.F, F4, Xp)) return rc;
        const RgradParams rp{dXh, xgate, Xp, H, F4, d.N, H, d.F, a->g_fc0_w, d.F, a->g_fc0_b, nullptr, nullptr};
        if (int rc = launch_rgrad(ctx, stream, rp)) return rc;
    } else if (a->g_fc0_w) {
        if (int rc = launch_gemm(stream, g, (d.N + 255) / 256)) return rc;
    } else if (a->g_fc0_b) {
        if (int rc = launch_colsum(stream, dXh, xgate, H, d.N, H, a->g_fc0_b, d.det)) return rc;
    }
    if (a->g_X) {
        GemmParams gx = gemm_input_grad(dXh, H, a->fc0_w, d.F, a->g_X, d.F, d.N, d.F, H);
        gx.gateA = xgate;
        if (int rc = launch_gemm(stream, gx)) return rc;
    }
    return PN_OK;
}

}  // namespace

extern "C" {

int pn_pagg_workspace_bytes(const pn_pagg_shape *shape, int64_t *bytes) {
    if (!shape || !bytes) PN_FAIL(PN_ERR_ARG, "pn_pagg_workspace_bytes: null");
    Dims d;
    if (int rc = make_dims(*shape, d)) return rc;
    *bytes = (int64_t)ws_layout(d).total;
    return PN_OK;
}

int pn_pagg_shape_info(const pn_pagg_shape *shape, int64_t out[4]) {
    if (!shape || !out) PN_FAIL(PN_ERR_ARG, "pn_pagg_shape_info: null");
    Dims d;
    if (int rc = make_dims(*shape, d)) return rc;
    out[0] = d.compact ? 1 : 0;
    out[1] = d.ZR;
    out[2] = d.nb;
    out[3] = d.math;
    return PN_OK;
}

int pn_pagg_paths_stream(pn_context *ctx, const pn_pagg_shape *shape, void *stream, void **out) {
    if (!shape || !out) PN_FAIL(PN_ERR_ARG, "pn_pagg_paths_stream: null");
    Dims d;
    if (int rc = make_dims(*shape, d)) return rc;
    // (run_tables: the plan of micro-batch 0 goes to the second stream unless every stage is timed; later micro-batches
    //  are planned on the caller's stream)
    void *side = (ctx && d.nb == 1 && !profiling_every_stage(ctx)) ? context_side_stream(ctx) : nullptr;
    *out = side ? side : stream;
    return PN_OK;
}

int pn_pagg_range_offset(const pn_pagg_shape *shape, int64_t *offset) {
    if (!shape || !offset) PN_FAIL(PN_ERR_ARG, "pn_pagg_range_offset: null");
    Dims d;
    if (int rc = make_dims(*shape, d)) return rc;
    static_assert(sizeof(SeqRange) == sizeof(pn_seq_range), "pn_seq_range is the public face of SeqRange");
    *offset = (d.math == PN_SEQ_MATH_F16X2 && d.G > 0 && !d.generic) ? (int64_t)ws_layout(d).range : -1;
    return PN_OK;
}

int pn_pagg_debug_offsets(const pn_pagg_shape *shape, int64_t out[4]) {
    if (!shape || !out) PN_FAIL(PN_ERR_ARG, "pn_pagg_debug_offsets: null");
    Dims d;
    if (int rc = make_dims(*shape, d)) return rc;
    const WsLayout w = ws_layout(d);
    out[0] = (int64_t)w.Xh;
    out[1] = (int64_t)w.Z;
    out[2] = (int64_t)w.hn;
    out[3] = (int64_t)w.layer1;
    return PN_OK;
}

int pn_pagg_forward(pn_context *ctx, const pn_pagg_args *a, void *stream) {
    return pn_pagg_forward_sparse(ctx, a, nullptr, stream);
}

int pn_pagg_forward_sparse(pn_context *ctx, const pn_pagg_args *a, const pn_sparse_features *sp, void *stream) {
    return pn_pagg_forward_weighted(ctx, a, sp, nullptr, stream);
}

int pn_pagg_forward_weighted(pn_context *ctx, const pn_pagg_args *a, const pn_sparse_features *sp, const pn_path_weights *pw,
                             void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    Call c;
    if (int rc = resolve_call(c, ctx, a, stream, "pn_pagg_forward", sp, pw)) return rc;
    const Dims &d = c.d;
    if (int rc = check_forward_args(c, "pn_pagg_forward")) return rc;
    if (d.S == 0) return PN_OK;
    JoinGuard joiner{ctx, stream};
    if (int rc = run_tables(c, joiner)) return rc;
    const bool save = d.nb == 1 && !a->no_save;  // several micro-batches: the backward re-runs each one's recurrence
    if (save && d.det)                           // the backward's scatter orders: second stream, under the recurrence
        if (int rc = fork_det_orders(c, joiner, 0)) return rc;
    for (int b = 0; b < d.nb; b++) {
        if (b > 0) {
            StageTimer tm(ctx, ST_PLAN_PACK, stream);
            if (int rc = run_plan(c, stream, b)) return rc;
        }
        if (int rc = run_seq_fwd(c, b, save)) return rc;
        if (int rc = run_pool_fwd(c, b, a->out + (size_t)b * d.Sb * d.C, true)) return rc;
    }
    return PN_OK;
}

// pn_pagg_backward, and -- with `target` -- pn_pagg_train_step: the forward of every micro-batch runs right before its
// backward (saved tensors in place), the loss gradient of its rows is formed in between
static int pagg_backward_impl(pn_context *ctx, const pn_pagg_args *a, void *stream_, const int64_t *target, float grad_scale,
                              float *loss, const pn_sparse_features *sp, const LossOpts *opts = nullptr,
                              float *denom_out = nullptr, const pn_path_weights *pw = nullptr,
                              const pn_path_grads *pg = nullptr) {
    hipStream_t stream = (hipStream_t)stream_;
    const bool fused = target != nullptr;
    // gradients at the per-path interface (pn_path_grads; all null: the call as it was)
    const float *g_pstate = pg ? pg->g_path_state : nullptr, *g_pweight = pg ? pg->g_path_weight : nullptr;
    float *g_weight = pg ? pg->g_weight : nullptr;
    if (g_weight && !(pw && pw->weight))
        PN_FAIL(PN_ERR_ARG, "%s: pn_path_grads.g_weight needs pn_path_weights.weight", fused ? "pn_pagg_train_step_paths" : "pn_pagg_backward_paths");
    Call c;
    if (int rc = resolve_call(c, ctx, a, stream, fused ? "pn_pagg_train_step" : "pn_pagg_backward", sp, pw)) return rc;
    const Dims &d = c.d;
    if (fused) {
        if (d.S > 0)
            if (int rc = check_forward_args(c, "pn_pagg_train_step")) return rc;
        // (one micro-batch: the loss kernel overwrites -- launch_cross_entropy zero-fills only if it needs several workgroups)
        if (d.nb > 1 || d.S == 0) PN_CHECK_HIP(hipMemsetAsync(loss, 0, sizeof(float), stream));
        // (pn_pagg_train_step_loss) D of the call's whole S rows, once, ahead of the micro-batches that all divide by it
        if (opts && denom_out && d.S > 0)
            if (int rc = launch_loss_denominator(target, d.S, d.C, *opts, denom_out, stream)) return rc;
    }
    // (S == 0 -- a rank of a sharded batch without masked nodes: its index arrays and g_out are empty tensors, i.e. NULL;
    //  the call still zero-fills every gradient it was given)
    if (!a->bank_w || !a->fc2_w || (d.S > 0 && (!a->ids || !a->codes || !a->sel || (!fused && !a->g_out && !a->g_embed && !g_pstate && !g_pweight))))
        PN_FAIL(PN_ERR_ARG, "pn_pagg_backward: null tensor");
    if (d.G > 0 && (!a->w_ih || !a->w_hh)) PN_FAIL(PN_ERR_ARG, "pn_pagg_backward: recurrent weights missing");
    if (!a->Xh_in && (!a->X || !a->fc0_w)) PN_FAIL(PN_ERR_ARG, "pn_pagg_backward: X / fc0 missing");
    if (a->Xh_in && !a->g_Xh) PN_FAIL(PN_ERR_ARG, "pn_pagg_backward: g_Xh is required with Xh_in");
    if (d.nb > 1 && !fused && ((d.G > 0 && (!a->b_ih || !a->b_hh)) || !a->fc2_b || (d.variant != PN_VARIANT_PAGG && !a->att_b)))
        PN_FAIL(PN_ERR_ARG, "pn_pagg_backward: micro-batches re-run the forward and need every forward tensor");
    const int H = d.H, L = d.L, GwH = d.Gw * H;     // GwH: rows of the caller's recurrent weights
    const bool has_att = d.variant != PN_VARIANT_PAGG;
    float *dZ = c.at<float>(c.w.dZ), *dXh = grad_xh(c);
    ZeroFill zf{ctx};
    if (int rc = zf.add(dZ, (size_t)d.ZR * H)) return rc;
    if (int rc = zf.add(dXh, (size_t)d.N * H)) return rc;
    if (int rc = zf.add(a->g_att_w, has_att ? (size_t)2 * H : 0)) return rc;
    if (int rc = zf.add(a->g_att_b, has_att ? 1 : 0)) return rc;
    if (has_att && (!a->g_att_w || !a->g_att_b))        // (pool_bwd_params: the attention gradients' stand-in)
        if (int rc = zf.add(c.at<float>(c.w.dl1), (size_t)2 * H + 1)) return rc;
    if (int rc = zf.add(a->g_fc2_b, (size_t)d.C)) return rc;
    if (int rc = zf.add(a->g_fc2_w, (size_t)d.C * 2 * H)) return rc;
    if (int rc = zf.add(a->g_bank_w, (size_t)L * H * H)) return rc;
    if (int rc = zf.add(a->g_bank_b, (size_t)L * H)) return rc;
    if (!a->Xh_in) {
        if (int rc = zf.add(a->g_fc0_w, (size_t)H * d.F)) return rc;
        if (int rc = zf.add(a->g_fc0_b, (size_t)H)) return rc;
    }
    if (d.S == 0) {
        if (int rc = zf.flush(stream)) return rc;
        if (int rc = zf.add(a->g_w_ih, (size_t)GwH * H)) return rc;
        if (int rc = zf.add(a->g_w_hh, (size_t)GwH * H)) return rc;
        if (int rc = zf.add(a->g_b_ih, (size_t)GwH)) return rc;
        if (int rc = zf.add(a->g_b_hh, (size_t)GwH)) return rc;
        if (int rc = zf.add(a->g_X, (size_t)d.N * d.F)) return rc;
        if (int rc = zf.flush(stream)) return rc;
        if (a->Xh_in && a->g_Xh_ready) PN_CHECK_HIP(hipEventRecord((hipEvent_t)a->g_Xh_ready, stream));    // (zeros: complete)
        return PN_OK;
    }
    JoinGuard joiner{ctx, stream};
    // (pn_pagg_train_step: the zero fill rides on the second stream with the index plan, joined before the recurrence -- off
    //  the chain recurrence -> pooling -> BPTT, where the forward's gigabyte of saved tensors would evict the freshly zeroed
    //  d Z: 7 MB to fetch again, ~1 us of HBM time, against 5 us of launch in the chain)
    if (int rc = fused ? run_tables(c, joiner, &zf) : zf.flush(stream)) return rc;
    // (per-stage timings are taken serially.  Deterministic mode: the classifier's weight gradient shares the chunk-sum
    //  buffer `dgemm` with the bank / fc0 backward and stays in line; the recurrent weight gradient goes to the second stream
    //  as in the default mode: run_wgrad)
    const bool side_ok = !profiling_every_stage(ctx) && !d.det;
    // pn_pagg_train_step, default mode: pooling forward + loss + pooling backward of a node as one launch (run_pool_step)
    const bool pool_step = fused && !d.det && knobs_of(ctx).pool_step != 0;
    if (d.det) {        // the identity the BPTT kernels index the contribution buffer with
        const int64_t n = std::max<int64_t>((int64_t)d.Sb * d.W * L, d.Sb);
        if (int rc = launch_det_iota(stream, c.at<int32_t>(c.w.iota), n)) return rc;
    }
    if (d.G > 0 && !d.generic) {
        StageTimer tm(ctx, ST_PLAN_PACK, stream);      // (its own bracket: ST_SEQ_BWD times the BPTT kernel alone)
        // (fp16: packed by the forward that left its saved tensors on this workspace -- run_pack_fwd, or run_tables above)
        if (d.math != PN_SEQ_MATH_F16X2)
            if (int rc = launch_pack_bwd3(stream, a->w_ih, a->w_hh, H, d.G, d.gru, c.at<void>(c.w.WpT))) return rc;
    }
    // Where the launches nothing waits for go -- the loss sum behind the pooling step, the classifier gradient and the attention
    // reduce (every fork / join is an event between two kernels of the queue and costs ~6 us of idle time there):
    //  - the recurrent weight gradient forks off behind the BPTT anyway: the three behind ONE fork after the pooling backward,
    //    on the second stream under the BPTT (profiles/r06_glue.txt sections 7 and 10);
    //  - mean / sum encoders, no recurrent gradient wanted, or no context: the classifier gradient (with the loss sum) forks
    //    on its own, ahead of the pooling backward or right behind the pooling step; the attention reduce stays in line;
    //  - deterministic mode or every stage timed: all three in line.
    const bool wgrad_wanted = d.G > 0 && (a->g_w_ih || a->g_w_hh || a->g_b_ih || a->g_b_hh);
    const bool small_behind_pool = side_ok && wgrad_wanted && ctx != nullptr;
    const bool rerun = fused || d.nb > 1;
    for (int b = 0; b < d.nb; b++) {
        const float *g_out = fused ? c.at<const float>(c.w.gout) : a->g_out ? a->g_out + (size_t)b * d.Sb * d.C : nullptr;
        float *loss_sum = pool_step ? loss : nullptr;
        if (rerun) {
            // pn_pagg_backward with micro-batches: this micro-batch's recurrence again (same seed and positions in the
            // batch -> same dropout masks), now keeping what the BPTT needs.  pn_pagg_train_step: its one and only
            // forward, the logits go to the caller, their loss gradient to the workspace.
            if (!(fused && b == 0)) {       // (run_tables made the plan of micro-batch 0)
                StageTimer tm(ctx, ST_PLAN_PACK, stream);
                if (int rc = run_plan(c, stream, b)) return rc;
            }
            if (d.det)                      // the scatters' destination orders: second stream, under this forward
                if (int rc = fork_det_orders(c, joiner, b)) return rc;
            if (int rc = run_seq_fwd(c, b, true)) return rc;
            if (!pool_step) {
                float *out_b = fused ? a->out + (size_t)b * d.Sb * d.C : c.at<float>(c.w.outb);
                if (int rc = run_pool_fwd(c, b, out_b)) return rc;
                if (fused)
                    if (int rc = launch_cross_entropy(out_b, target + (size_t)b * d.Sb, c.groups(b), d.C, grad_scale, loss,
                                                      c.at<float>(c.w.gout), stream, d.nb == 1, opts))
                        return rc;
            }
        }
        PoolBwdParams pp = pool_bwd_params(c, b, g_out);
        if (a->g_embed) pp.g_embed = a->g_embed + (size_t)b * d.Sb * 2 * H;     // (never with the pooling step: train_step refuses it)
        if (g_pstate) pp.g_state = g_pstate + (size_t)b * d.Sb * d.W * H;       // (rows of the call's groups, like out_path_state)
        if (g_pweight) pp.g_coef = g_pweight + (size_t)b * d.Sb * d.W;
        pp.d_omega = g_weight;      // (indexed by slot like omega: no row offset)
        if (pool_step)
            if (int rc = run_pool_step(c, b, pp, target, grad_scale, opts)) return rc;
        if (!small_behind_pool)
            if (int rc = run_fc2_grad(c, b, joiner, fork_if(c, side_ok), g_out, loss_sum, grad_scale, opts)) return rc;
        if (int rc = run_pool_bwd(c, pp, pool_step)) return rc;
        const hipStream_t small = fork_if(c, small_behind_pool);
        if (small_behind_pool)
            if (int rc = run_fc2_grad(c, b, joiner, small, g_out, loss_sum, grad_scale, opts)) return rc;
        if (int rc = run_att_reduce(c, joiner, small, pp)) return rc;
        if (d.det) {
            // (this micro-batch's orders were sorted on the second stream under its forward, when the backward re-ran it)
            if (rerun)
                if (int rc = joiner.join()) return rc;
            if (int rc = run_pool_scatters(c, b, pp)) return rc;
        }
        if (int rc = run_seq_bwd(c, b)) return rc;
        if (wgrad_wanted)
            if (int rc = run_wgrad(c, b, joiner)) return rc;
        // the next micro-batch rewrites the [x|h] rows and dG the weight-gradient GEMM is reading
        if (b + 1 < d.nb)
            if (int rc = joiner.join()) return rc;
    }
    if (int rc = run_bank_bwd(c, dXh, dZ)) return rc;
    if (a->Xh_in) return PN_OK;   // the caller finishes fc0 after the reduce-scatter of g_Xh
    return run_fc0_bwd(c, dXh);
}

// what every training-step entry point asks of its arguments before it looks at the shape
static int check_train_step_args(const pn_pagg_args *a, const int64_t *target, const float *loss, const char *who) {
    if (!a) PN_FAIL(PN_ERR_ARG, "%s: null args", who);
    if (a->out_embed || a->out_path_weight || a->out_path_state || a->g_embed)
        PN_FAIL(PN_ERR_ARG, "%s: out_embed / out_path_weight / out_path_state / g_embed are for pn_pagg_forward / pn_pagg_backward", who);
    if (!loss || (a->shape.S > 0 && !target)) PN_FAIL(PN_ERR_ARG, "%s: null target / loss", who);
    return PN_OK;
}

int pn_pagg_backward(pn_context *ctx, const pn_pagg_args *a, void *stream) {
    return pagg_backward_impl(ctx, a, stream, nullptr, 0.0f, nullptr, nullptr);
}

int pn_pagg_backward_sparse(pn_context *ctx, const pn_pagg_args *a, const pn_sparse_features *sp, void *stream) {
    return pagg_backward_impl(ctx, a, stream, nullptr, 0.0f, nullptr, sp);
}

int pn_pagg_backward_weighted(pn_context *ctx, const pn_pagg_args *a, const pn_sparse_features *sp, const pn_path_weights *pw,
                              void *stream) {
    return pagg_backward_impl(ctx, a, stream, nullptr, 0.0f, nullptr, sp, nullptr, nullptr, pw);
}

int pn_pagg_train_step(pn_context *ctx, const pn_pagg_args *a, const int64_t *target, float grad_scale, float *loss,
                       void *stream) {
    return pn_pagg_train_step_sparse(ctx, a, nullptr, target, grad_scale, loss, stream);
}

int pn_pagg_train_step_sparse(pn_context *ctx, const pn_pagg_args *a, const pn_sparse_features *sp, const int64_t *target,
                              float grad_scale, float *loss, void *stream) {
    return pn_pagg_train_step_weighted(ctx, a, sp, nullptr, target, grad_scale, loss, stream);
}

int pn_pagg_train_step_weighted(pn_context *ctx, const pn_pagg_args *a, const pn_sparse_features *sp, const pn_path_weights *pw,
                                const int64_t *target, float grad_scale, float *loss, void *stream) {
    if (int rc = check_train_step_args(a, target, loss, "pn_pagg_train_step")) return rc;
    if (a->shape.S == 0) {          // nothing to aggregate: zero loss, zero gradients
        PN_CHECK_HIP(hipMemsetAsync(loss, 0, sizeof(float), (hipStream_t)stream));
        return pagg_backward_impl(ctx, a, stream, nullptr, 0.0f, nullptr, sp);
    }
    return pagg_backward_impl(ctx, a, stream, target, grad_scale, loss, sp, nullptr, nullptr, pw);
}

int pn_pagg_train_step_loss(pn_context *ctx, const pn_pagg_args *a, const pn_sparse_features *sp, const pn_loss_spec *spec,
                            const int64_t *target, float *loss, void *stream) {
    return pn_pagg_train_step_loss_weighted(ctx, a, sp, spec, nullptr, target, loss, stream);
}

int pn_pagg_train_step_loss_weighted(pn_context *ctx, const pn_pagg_args *a, const pn_sparse_features *sp, const pn_loss_spec *spec,
                                     const pn_path_weights *pw, const int64_t *target, float *loss, void *stream) {
    LossOpts o;
    if (int rc = loss_opts_from_spec(spec, "pn_pagg_train_step_loss", &o)) return rc;
    if (int rc = check_train_step_args(a, target, loss, "pn_pagg_train_step_loss")) return rc;
    float *denom_out = spec->denominator_given ? nullptr : spec->denominator;
    if (a->shape.S == 0) {          // nothing to aggregate: zero loss, zero gradients (and D = 0, when it is this call's to write)
        PN_CHECK_HIP(hipMemsetAsync(loss, 0, sizeof(float), (hipStream_t)stream));
        if (denom_out) PN_CHECK_HIP(hipMemsetAsync(denom_out, 0, sizeof(float), (hipStream_t)stream));
        return pagg_backward_impl(ctx, a, stream, nullptr, 0.0f, nullptr, sp);
    }
    return pagg_backward_impl(ctx, a, stream, target, o.grad_scale, loss, sp, &o, denom_out, pw);
}

int pn_pagg_backward_paths(pn_context *ctx, const pn_pagg_args *a, const pn_sparse_features *sp, const pn_path_weights *pw,
                           const pn_path_grads *pg, void *stream) {
    return pagg_backward_impl(ctx, a, stream, nullptr, 0.0f, nullptr, sp, nullptr, nullptr, pw, pg);
}

int pn_pagg_train_step_paths(pn_context *ctx, const pn_pagg_args *a, const pn_sparse_features *sp, const pn_loss_spec *spec,
                             const pn_path_weights *pw, const pn_path_grads *pg, const int64_t *target, float grad_scale,
                             float *loss, void *stream) {
    // (before the device is looked at, like out_embed in check_train_step_args)
    if (pg && (pg->g_path_state || pg->g_path_weight))
        PN_FAIL(PN_ERR_ARG, "pn_pagg_train_step_paths: g_path_state / g_path_weight are for pn_pagg_backward_paths");
    if (pg && pg->g_weight && !(pw && pw->weight))
        PN_FAIL(PN_ERR_ARG, "pn_pagg_train_step_paths: pn_path_grads.g_weight needs pn_path_weights.weight");
    LossOpts o;
    if (spec)
        if (int rc = loss_opts_from_spec(spec, "pn_pagg_train_step_paths", &o)) return rc;
    if (int rc = check_train_step_args(a, target, loss, "pn_pagg_train_step_paths")) return rc;
    float *denom_out = spec && !spec->denominator_given ? spec->denominator : nullptr;
    if (a->shape.S == 0) {          // nothing to aggregate: zero loss, zero gradients; g_weight has no entry of this call's
        PN_CHECK_HIP(hipMemsetAsync(loss, 0, sizeof(float), (hipStream_t)stream));
        if (denom_out) PN_CHECK_HIP(hipMemsetAsync(denom_out, 0, sizeof(float), (hipStream_t)stream));
        return pagg_backward_impl(ctx, a, stream, nullptr, 0.0f, nullptr, sp);
    }
    if (spec) return pagg_backward_impl(ctx, a, stream, target, o.grad_scale, loss, sp, &o, denom_out, pw, pg);
    return pagg_backward_impl(ctx, a, stream, target, grad_scale, loss, sp, nullptr, nullptr, pw, pg);
}

}  // extern "C"

