// pn_explain.hip -- exact path and group occlusion of a prediction (pn_explain_groups / pn_explain_overlap /
// pn_explain_totals).
//
// The recurrence never sees the pooling, and the classifier is linear after it: what the model would say without a set of a
// row's members, or with that set alone, is a closed form over the members' final hidden states (include/pathnet_hip.h has
// the definition).  This file evaluates it for all groups of all rows in one pass over `state`.
//
//   explain_kernel<LANES, OVERLAP>  one workgroup owns a row.  Per class chunk: the row's [W, H] states, its ego row and the two
//                             halves of fc2's rows go through LDS in tiles of Ht hidden units (16-byte loads where the
//                             addresses allow), and thread (j, c) adds its products in ascending h into con[j, c] (fp64, LDS;
//                             row W is the ego's e[c]).  Then LANES threads own one logit vector at a time -- drop_g, keep_g,
//                             full, e -- form it class by class (members in ascending j) and keep a running (max, sum of
//                             exp, value at the target, argmax); the lanes' maxima meet in a butterfly, every lane rescales
//                             its sum once, and the sums meet in a butterfly.
//   explain_totals_kernel     one workgroup owns a group: 256 rows are fetched at a time, thread 0 adds them in ascending
//                             order in fp64 and adds once into the running total; the integer totals are exact.
//
// Work split (pn_explain_route):
//   lanes        8 for C <= 8, 16 for C <= 16, else 64: the threads that share a logit vector
//   class chunk  Cc = min(C, 4096 / (W + 1)): con holds (W + 1) * Cc doubles.  One chunk (the hot case): `state` is read from
//                memory once.  More (W + 1) * C > 4096): the H loop is run once per chunk and the vectors' running
//                values are carried from chunk to chunk in LDS.
//   H tile       the largest Ht with (W + 1 + 2 Cc) * (Ht | 1) <= 7168 floats, a multiple of 4 when it is below H; rows of the
//                tile are Ht | 1 floats apart, so that neighbouring threads' rows start in different banks.
// Overlapping groups (pn_explain_overlap): the same kernel body with OVERLAP = true.  A member then carries M labels instead of
// one group id, and "member j is in group g" is M compares against label[j, 0 .. M) in LDS (W * M <= 1024 ints, 4 KB) where
// the partition kernel makes one.  The alternative, a bit table [W, G / 32] in LDS, was not taken: at the cap (W = 1024,
// M = 1, G = 1024) it is 128 KB and does not fit beside the 152 KB plan below, so it could only ever be a second path with a
// size threshold; and the compares cost no LDS bandwidth worth saving -- every lane of a wave reads the SAME label word (the
// lanes differ in g and c only), which the LDS serves as one broadcast per instruction, conflict-free, and the loop's other
// read (con[j, cc], 8 bytes a lane) dominates.  The work per row is (2 G + 2) C W M compares: 3.6e5 at the hot node shape
// (W = 40, M = 4, G = 160, C = 7).  OVERLAP = false keeps pn_explain_groups' instructions: the predicate is a template
// parameter, not a run-time branch.
// LDS at G = 1024 (NV = 2050 vectors): rho, vm, vz, vx 4 * 16400 + vb, mode 2 * 8208 + con <= 32768 + grp <= 4096 + pres 4096
// + label <= 4096 + tile <= 28672 = at most 155744 bytes (+ 256 static; the largest plan_of found over the shapes on both
// sides of every boundary is 152480) of gfx950's 163840 (160 KiB) per workgroup; one workgroup a CU there, which the partition
// kernel at G = 1024 already is.
// Every sum's order is a function of (W, H, C, G, M) alone -- not of S, the grid, or the rows next to it -- and there is no
// floating-point atomic.  A product of two converted fp32 values is exact in fp64, so the dot products round in their
// additions only.  Plain C++ and vector stores only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pn_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1 << 16;      // rows (groups) beyond that are taken in a grid-stride loop
constexpr int kMaxCon = 4096;            // doubles of con: (W + 1) * Cc
constexpr int kTileFloats = 7168;        // floats of one H tile: (W + 1 + 2 Cc) * (Ht | 1)
constexpr int kMaxW = 1024, kMaxG = 1024, kMaxH = 4096, kMaxC = 1024;
constexpr int kMaxM = 16, kMaxLabels = 1024;      // pn_explain_overlap: labels per member, and per row (W * M)

// how a logit vector picks its members
constexpr int kModeZero = 0;             // pooled part zero: x = e
constexpr int kModeRest = 1;             // live members outside group g
constexpr int kModeGroup = 2;            // live members of group g
constexpr int kModeAll = 3;              // every member (full; drop of an empty group)

struct Plan {
    int32_t route, lanes, Cc, Ht, ldt;
    int32_t off_con, off_rho, off_vm, off_vz, off_vx, off_vb, off_mode, off_grp, off_pres, off_lab, off_tile, bytes;
};

struct Params {
    int64_t S;
    int32_t W, H, C, G, M;       // M: labels per member (pn_explain_overlap), 0 for a partition
    const float *state;
    int64_t ld_state;
    const float *coef, *ego;
    int64_t ld_ego;
    const float *w;
    int64_t ld_w;
    const float *b, *weight;
    const int32_t *group;       // [S, W], or [S, W, M] labels
    int32_t norm, renorm;
    const int64_t *target;
    pn_explain_out o;
    int32_t *status;
    Plan pl;
};

__device__ inline bool finite32(float v) { return fabsf(v) <= 3.4028234663852886e38f; }     // false for NaN and both infinities

// `nrows` rows of `ht` floats, row r at src + r * src_ld, into dst + r * ldt.  -> 1 when a value read is not finite
__device__ inline int load_rows(float *dst, int ldt, const float *src, int64_t src_ld, int nrows, int ht) {
    const bool vec = ((uintptr_t)src & 15) == 0 && (src_ld & 3) == 0;
    const int q = (ht + 3) >> 2;
    int bad = 0;
    for (int i = threadIdx.x; i < nrows * q; i += kThreads) {
        const int r = i / q, h = (i - r * q) << 2;
        const float *p = src + (int64_t)r * src_ld + h;
        float *d = dst + r * ldt + h;
        if (vec && h + 4 <= ht) {
            const float4 v = *(const float4 *)p;
            d[0] = v.x;
            d[1] = v.y;
            d[2] = v.z;
            d[3] = v.w;
            bad |= !(finite32(v.x) && finite32(v.y) && finite32(v.z) && finite32(v.w));
        } else {
            for (int k = 0; k < 4 && h + k < ht; k++) {
                const float v = p[k];
                d[k] = v;
                bad |= !finite32(v);
            }
        }
    }
    return bad;
}

// running values of a logit vector: m = max, z = sum exp(x - m), x = the value at the target (0 where not seen), b = the
// lowest class that holds m.  Joins what one class chunk left with the next chunk's.
__device__ inline void merge(double &m, double &z, double &x, int32_t &b, double m2, double z2, double x2, int32_t b2) {
    if (m2 > m || (m2 == m && b2 < b)) b = b2;
    if (m2 == -INFINITY) {
    } else if (m == -INFINITY) {
        m = m2;
        z = z2;
    } else if (m >= m2) {
        z = z + z2 * exp(m2 - m);
    } else {
        z = z2 + z * exp(m - m2);
        m = m2;
    }
    x += x2;
}

// is live member j in group g?  A partition: its one id.  Overlapping groups: any of its M labels (a repeated label counts
// once; a label outside [0, G) equals no g).  grp[j] is >= 0 for a live member in both.
template <bool OVERLAP>
__device__ inline int member_in(const int32_t *grp, const int32_t *lab, int32_t M, int32_t j, int32_t g) {
    if (!OVERLAP) return grp[j] == g;
    int in = 0;
    for (int32_t m = 0; m < M; m++) in |= lab[j * M + m] == g;
    return in;
}

template <int LANES, bool OVERLAP>
__global__ __launch_bounds__(kThreads) void explain_kernel(Params p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Plan &pl = p.pl;
    double *con = (double *)(smem + pl.off_con);        // [(W + 1), cc_n]
    double *rho = (double *)(smem + pl.off_rho);        // [2G + 2]: drop 0 .. G-1, keep G .. 2G-1, full, e
    double *vm = (double *)(smem + pl.off_vm);
    double *vz = (double *)(smem + pl.off_vz);
    double *vx = (double *)(smem + pl.off_vx);
    int32_t *vb = (int32_t *)(smem + pl.off_vb);
    int32_t *mode = (int32_t *)(smem + pl.off_mode);
    int32_t *grp = (int32_t *)(smem + pl.off_grp);      // [W]: -1 dead, g, or G for a live member of no group
    int32_t *pres = (int32_t *)(smem + pl.off_pres);    // [G]
    int32_t *lab = (int32_t *)(smem + pl.off_lab);      // [W, M] with OVERLAP: a dead member's are -1
    float *tile = (float *)(smem + pl.off_tile);
    double *wl = (double *)tile, *cf = wl + p.W;        // live weights and coefficients: done with before the first tile
    const int32_t W = p.W, H = p.H, C = p.C, G = p.G, M = p.M, Cc = pl.Cc, Ht = pl.Ht, ldt = pl.ldt;
    const int32_t NV = 2 * G + 2, VFULL = 2 * G;
    const int32_t nchunks = (C + Cc - 1) / Cc;
    const int tid = threadIdx.x;
    const int sub = tid / LANES, lane = tid % LANES, nsub = kThreads / LANES;
    const pn_explain_out &o = p.o;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);

    for (int64_t s = blockIdx.x; s < p.S; s += gridDim.x) {
        int bad = 0;
        // ---- members ----------------------------------------------------------------------------------------------------
        for (int32_t j = tid; j < W; j += kThreads) {
            const float c = p.coef[s * W + j];
            bad |= !finite32(c);
            const float wv = p.weight ? p.weight[s * W + j] : 1.0f;
            const bool live = finite32(wv) && wv > 0.0f;
            if (OVERLAP) {
                grp[j] = live ? 0 : -1;
                for (int32_t m = 0; m < M; m++) lab[j * M + m] = live ? p.group[(s * W + j) * M + m] : -1;
            } else {
                const int32_t gi = p.group[s * W + j];
                grp[j] = live ? (gi >= 0 && gi < G ? gi : G) : -1;
            }
            wl[j] = live ? (double)wv : 0.0;
            cf[j] = live ? (double)c : 0.0;
        }
        for (int32_t c = tid; c < C; c += kThreads) bad |= !finite32(p.b[c]);
        __syncthreads();
        // ---- groups: the sums by direct summation in ascending j, the factors, the member selection --------------------
        for (int32_t g = tid; g < G; g += kThreads) {
            double Om = 0.0, K = 0.0, OmR = 0.0, KR = 0.0, OmX = 0.0, KX = 0.0;
            int32_t nR = 0, nX = 0;
            // (branch-free, so that the unrolled loop's LDS reads run ahead of the sums: a member left out adds +0.0, which
            //  changes no bit; wl and cf are 0 for a dead member)
#pragma unroll 8
            for (int32_t j = 0; j < W; j++) {
                const int32_t gj = grp[j];
                const double wj = wl[j], cj = cf[j];
                const bool in = member_in<OVERLAP>(grp, lab, M, j, g), out = gj >= 0 && !in;
                Om += wj;
                K += cj;
                OmR += in ? wj : 0.0;
                KR += in ? cj : 0.0;
                OmX += out ? wj : 0.0;
                KX += out ? cj : 0.0;
                nR += in;
                nX += out;
            }
            pres[g] = nR;
            int32_t md = kModeZero, mk = kModeZero;
            double rd = 0.0, rk = 0.0;
            if (nR == 0) {
                md = kModeAll;
                rd = 1.0;
            } else if (nX > 0 && !(p.renorm && !(KX > 0.0))) {
                md = kModeRest;
                rd = (p.norm == PN_PATH_NORM_SUM ? Om / OmX : 1.0) * (p.renorm ? K / KX : 1.0);
            }
            if (nR > 0 && !(p.renorm && !(KR > 0.0))) {
                mk = kModeGroup;
                rk = (p.norm == PN_PATH_NORM_SUM ? Om / OmR : 1.0) * (p.renorm ? K / KR : 1.0);
            }
            mode[g] = md;
            rho[g] = rd;
            mode[G + g] = mk;
            rho[G + g] = rk;
        }
        if (tid == 0) {
            mode[VFULL] = kModeAll;
            rho[VFULL] = 1.0;
            mode[VFULL + 1] = kModeZero;
            rho[VFULL + 1] = 0.0;
        }
        int64_t t = p.target ? p.target[s] : -1;
        const int first_pass = p.target ? 1 : 0;        // without a target, pass 0 finds the argmax of the full logits
        __syncthreads();

        for (int pass = first_pass; pass < 2; pass++) {
            for (int32_t v = tid; v < NV; v += kThreads) {
                vm[v] = -INFINITY;
                vz[v] = 0.0;
                vx[v] = 0.0;
                vb[v] = C;
            }
            for (int32_t ch = 0; ch < nchunks; ch++) {
                const int32_t c0 = ch * Cc, cc_n = C - c0 < Cc ? C - c0 : Cc;
                if (pass == first_pass || nchunks > 1) {        // (a single chunk's con is still there in pass 1)
                    // ---- con[j, c] = sum_h fc2_w[c, H + h] state[j, h];  con[W, c] = sum_h fc2_w[c, h] ego[h] ------------
                    float *t_ego = tile + W * ldt, *t_wp = tile + (W + 1) * ldt, *t_we = t_wp + Cc * ldt;
                    for (int32_t h0 = 0; h0 < H; h0 += Ht) {
                        const int32_t ht = H - h0 < Ht ? H - h0 : Ht;
                        __syncthreads();
                        bad |= load_rows(tile, ldt, p.state + s * W * p.ld_state + h0, p.ld_state, W, ht);
                        bad |= load_rows(t_ego, ldt, p.ego + s * p.ld_ego + h0, p.ld_ego, 1, ht);
                        bad |= load_rows(t_wp, ldt, p.w + (int64_t)c0 * p.ld_w + H + h0, p.ld_w, cc_n, ht);
                        bad |= load_rows(t_we, ldt, p.w + (int64_t)c0 * p.ld_w + h0, p.ld_w, cc_n, ht);
                        __syncthreads();
                        for (int32_t i = tid; i < (W + 1) * cc_n; i += kThreads) {
                            const int32_t j = i / cc_n, cc = i - j * cc_n;
                            const float *x = tile + j * ldt, *wr = (j < W ? t_wp : t_we) + cc * ldt;
                            double acc = h0 ? con[i] : 0.0;
#pragma unroll 8
                            for (int32_t h = 0; h < ht; h++) acc = fma((double)x[h], (double)wr[h], acc);
                            con[i] = acc;
                        }
                    }
                    __syncthreads();
                    // ---- contribution = coef t / W;  e = b + dot -----------------------------------------------------------
                    const bool write = pass == 1 || nchunks == 1;
                    for (int32_t i = tid; i < (W + 1) * cc_n; i += kThreads) {
                        const int32_t j = i / cc_n, cc = i - j * cc_n;
                        if (j < W) {
                            const double v = (double)p.coef[s * W + j] * con[i] / (double)W;
                            con[i] = v;
                            if (write && o.contribution) o.contribution[(s * W + j) * C + c0 + cc] = (float)v;
                        } else {
                            con[i] = (double)p.b[c0 + cc] + con[i];
                        }
                    }
                }
                __syncthreads();
                // ---- the logit vectors: LANES threads own one at a time ------------------------------------------------------
                const int32_t v_begin = pass == 0 ? VFULL : 0, v_end = pass == 0 ? VFULL + 1 : NV;
                for (int32_t v = v_begin + sub; v < v_end; v += nsub) {
                    const int32_t md = mode[v], g = v < G ? v : v - G;
                    const double r = rho[v];
                    double m = -INFINITY, z = 0.0, xt = 0.0;
                    int32_t bc = C;
                    for (int32_t cc = lane; cc < cc_n; cc += LANES) {
                        const int32_t c = c0 + cc;
                        double x = con[W * cc_n + cc];
                        if (md != kModeZero) {
                            double sum = 0.0;
                            // (no branch in the loop: its LDS reads run ahead of the sum; +0.0 changes no bit)
                            const int f_all = md == kModeAll, f_grp = md == kModeGroup, f_rest = md == kModeRest;
#pragma unroll 8
                            for (int32_t j = 0; j < W; j++) {
                                const int32_t gj = grp[j];
                                const double term = con[j * cc_n + cc];
                                const int in = member_in<OVERLAP>(grp, lab, M, j, g), live = gj >= 0;
                                const int take = f_all | (f_grp & in) | (f_rest & live & (in ^ 1));
                                sum += take ? term : 0.0;
                            }
                            x = fma(r, sum, x);
                        }
                        if (pass == 1) {
                            if (v < G) {
                                if (o.drop_logits) o.drop_logits[(s * G + g) * C + c] = (float)x;
                            } else if (v < VFULL) {
                                if (o.keep_logits) o.keep_logits[(s * G + g) * C + c] = (float)x;
                            } else if (v == VFULL) {
                                if (o.full) o.full[s * C + c] = (float)x;
                            }
                        }
                        // (the lane's running max and sum; its first class costs no exp)
                        if (x > m) {
                            z = z == 0.0 ? 1.0 : fma(z, exp(m - x), 1.0);
                            bc = c;
                            m = x;
                        } else {
                            z += exp(x - m);
                        }
                        if (c == t) xt = x;
                    }
                    // the lanes' maxima meet in a butterfly (the lowest class among equals), every lane rescales its sum once,
                    // and the sums meet in a butterfly: one exp per lane, and every lane ends with the same bits
                    double mx = m;
                    int32_t bx = bc;
#pragma unroll
                    for (int mask = LANES / 2; mask >= 1; mask >>= 1) {
                        const double m2 = __shfl_xor(mx, mask, LANES);
                        const int32_t b2 = __shfl_xor(bx, mask, LANES);
                        if (m2 > mx || (m2 == mx && b2 < bx)) bx = b2;
                        mx = m2 > mx ? m2 : mx;
                    }
                    z = m == mx ? z : z * exp(m - mx);          // (an idle lane: m = -inf, z = 0)
#pragma unroll
                    for (int mask = LANES / 2; mask >= 1; mask >>= 1) {
                        z += __shfl_xor(z, mask, LANES);
                        xt += __shfl_xor(xt, mask, LANES);
                    }
                    m = mx;
                    bc = bx;
                    if (lane == 0 && ch > 0) merge(m, z, xt, bc, vm[v], vz[v], vx[v], vb[v]);
                    if (lane == 0) {
                        vm[v] = m;
                        vz[v] = z;
                        vx[v] = xt;
                        vb[v] = bc;
                    }
                }
            }
            __syncthreads();
            if (pass == 0) {
                t = vb[VFULL];
                __syncthreads();
            }
        }

        // ---- scores --------------------------------------------------------------------------------------------------------
        const int badrow = __syncthreads_or(bad);
        const bool t_ok = t >= 0 && t < C;
        for (int32_t g = tid; g < G; g += kThreads) {
            double dd = 0.0, kg = 0.0;
            int32_t fl = 0;
            if (badrow) {
                dd = kg = nan;
            } else if (t_ok) {
                const double lp_full = vx[VFULL] - (vm[VFULL] + log(vz[VFULL]));
                const double lp_e = vx[VFULL + 1] - (vm[VFULL + 1] + log(vz[VFULL + 1]));
                const double lp_drop = vx[g] - (vm[g] + log(vz[g]));
                const double lp_keep = vx[G + g] - (vm[G + g] + log(vz[G + g]));
                dd = lp_full - lp_drop;
                kg = lp_keep - lp_e;
                fl = pres[g] > 0 && vb[g] != vb[VFULL];
            }
            if (o.drop_delta) o.drop_delta[s * G + g] = (float)dd;
            if (o.keep_gain) o.keep_gain[s * G + g] = (float)kg;
            if (o.flip) o.flip[s * G + g] = (uint8_t)fl;
            if (o.present) o.present[s * G + g] = pres[g];
        }
        if (tid == 0) {
            if (o.target_used) o.target_used[s] = badrow && !p.target ? -1 : t;
            if (p.status) {
                if (badrow) atomicAdd(p.status + 1, 1);
                else if (!t_ok) atomicAdd(p.status, 1);
            }
        }
        if (badrow) {
            const float nanf = __int_as_float(0x7fc00000);
            if (o.full)
                for (int32_t i = tid; i < C; i += kThreads) o.full[s * C + i] = nanf;
            if (o.contribution)
                for (int32_t i = tid; i < W * C; i += kThreads) o.contribution[s * W * C + i] = nanf;
            for (int32_t i = tid; i < G * C; i += kThreads) {
                if (o.drop_logits) o.drop_logits[s * G * C + i] = nanf;
                if (o.keep_logits) o.keep_logits[s * G * C + i] = nanf;
            }
        }
        __syncthreads();        // the next row reuses the LDS
    }
}

// ---- totals ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void explain_totals_kernel(int64_t S, int32_t G, const float *drop_delta,
                                                                   const float *keep_gain, const uint8_t *flip,
                                                                   const int32_t *present, const int32_t *rows, int64_t n,
                                                                   void *totals) {
    __shared__ double sd[kThreads], sk[kThreads];
    __shared__ long long si[3][kThreads / 64];
    long long *rows_present = (long long *)totals, *members = rows_present + G, *flips = members + G;
    double *dd_sum = (double *)(flips + G), *kg_sum = dd_sum + G;
    const int tid = threadIdx.x;
    for (int32_t g = blockIdx.x; g < G; g += gridDim.x) {
        long long n_rows = 0, n_mem = 0, n_flip = 0;
        double acc_d = 0.0, acc_k = 0.0;        // thread 0's
        for (int64_t base = 0; base < n; base += kThreads) {
            const int64_t i = base + tid;
            double d = 0.0, k = 0.0;
            if (i < n) {
                const int64_t row = rows ? (int64_t)rows[i] : i;
                if (row >= 0 && row < S) {
                    const int32_t pr = present[row * G + g];
                    const float fd = drop_delta[row * G + g], fk = keep_gain[row * G + g];
                    if (pr > 0 && finite32(fd) && finite32(fk)) {
                        d = (double)fd;
                        k = (double)fk;
                        n_rows += 1;
                        n_mem += pr;
                        n_flip += flip[row * G + g] != 0;
                    }
                }
            }
            __syncthreads();        // thread 0 is done with the previous batch
            sd[tid] = d;
            sk[tid] = k;
            __syncthreads();
            if (tid == 0) {
                // (a row left out adds +0.0, which changes no bit of a sum that started at +0.0)
                const int cnt = n - base < kThreads ? (int)(n - base) : kThreads;
#pragma unroll 16
                for (int r = 0; r < cnt; r++) {
                    acc_d += sd[r];
                    acc_k += sk[r];
                }
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            n_rows += __shfl_xor(n_rows, m, 64);
            n_mem += __shfl_xor(n_mem, m, 64);
            n_flip += __shfl_xor(n_flip, m, 64);
        }
        __syncthreads();
        if ((tid & 63) == 0) {
            si[0][tid >> 6] = n_rows;
            si[1][tid >> 6] = n_mem;
            si[2][tid >> 6] = n_flip;
        }
        __syncthreads();
        if (tid == 0) {
            rows_present[g] += si[0][0] + si[0][1] + si[0][2] + si[0][3];
            members[g] += si[1][0] + si[1][1] + si[1][2] + si[1][3];
            flips[g] += si[2][0] + si[2][1] + si[2][2] + si[2][3];
            dd_sum[g] += acc_d;
            kg_sum[g] += acc_k;
        }
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
int check_shape(const char *who, int64_t S, int32_t W, int32_t H, int32_t C, int32_t G) {
    if (S < 0 || S > 2147483647LL) PN_FAIL(PN_ERR_ARG, "%s: %lld rows, 0 .. 2^31 - 1", who, (long long)S);
    if (W < 1 || W > kMaxW) PN_FAIL(PN_ERR_ARG, "%s: %d members, 1 .. %d", who, W, kMaxW);
    if (G < 1 || G > kMaxG) PN_FAIL(PN_ERR_ARG, "%s: %d groups, 1 .. %d", who, G, kMaxG);
    if (H < 1 || H > kMaxH) PN_FAIL(PN_ERR_ARG, "%s: hidden size %d, 1 .. %d", who, H, kMaxH);
    if (C < 1 || C > kMaxC) PN_FAIL(PN_ERR_ARG, "%s: %d classes, 1 .. %d", who, C, kMaxC);
    return PN_OK;
}

int32_t align16(int32_t v) { return (v + 15) & ~15; }

// M: labels per member, 0 for a partition (no label array: pn_explain_groups' plan to the byte)
Plan plan_of(int64_t S, int32_t W, int32_t H, int32_t C, int32_t G, int32_t M = 0) {
    Plan pl{};
    pl.lanes = C <= 8 ? 8 : C <= 16 ? 16 : 64;
    const int32_t fit = kMaxCon / (W + 1);
    pl.Cc = C < fit ? C : fit;
    const int32_t per = W + 1 + 2 * pl.Cc;
    int32_t Ht = 1;
    while (Ht < H && (int64_t)per * ((Ht + 1) | 1) <= kTileFloats) Ht++;
    if (Ht < H && Ht >= 4) Ht &= ~3;
    pl.Ht = Ht;
    pl.ldt = Ht | 1;
    pl.route = S == 0 ? PN_EXPLAIN_ROUTE_NONE : pl.Cc == C ? PN_EXPLAIN_ROUTE_ROW : PN_EXPLAIN_ROUTE_CHUNKED;
    const int32_t NV = 2 * G + 2;
    int32_t off = 0;
    pl.off_con = off;
    off = align16(off + 8 * (W + 1) * pl.Cc);
    pl.off_rho = off;
    off = align16(off + 8 * NV);
    pl.off_vm = off;
    off = align16(off + 8 * NV);
    pl.off_vz = off;
    off = align16(off + 8 * NV);
    pl.off_vx = off;
    off = align16(off + 8 * NV);
    pl.off_vb = off;
    off = align16(off + 4 * NV);
    pl.off_mode = off;
    off = align16(off + 4 * NV);
    pl.off_grp = off;
    off = align16(off + 4 * W);
    pl.off_pres = off;
    off = align16(off + 4 * G);
    pl.off_lab = off;
    off = align16(off + 4 * W * M);
    pl.off_tile = off;
    const int32_t tile_bytes = 4 * per * pl.ldt, member_bytes = 16 * W;
    pl.bytes = align16(off + (tile_bytes > member_bytes ? tile_bytes : member_bytes));
    return pl;
}

unsigned blocks_for(int64_t n) { return (unsigned)(n < kMaxBlocks ? n : kMaxBlocks); }

template <bool OVERLAP>
int launch_explain(pn_context *ctx, const Params &p, hipStream_t stream) {
    const void *kernel = p.pl.lanes == 8 ? (const void *)explain_kernel<8, OVERLAP>
                                         : p.pl.lanes == 16 ? (const void *)explain_kernel<16, OVERLAP>
                                                            : (const void *)explain_kernel<64, OVERLAP>;
    if (p.pl.bytes > 65536)
        if (int rc = pn::ensure_dynamic_lds(ctx, kernel, p.pl.bytes)) return rc;
    const dim3 grid(blocks_for(p.S)), block(kThreads);
    if (p.pl.lanes == 8)
        hipLaunchKernelGGL((explain_kernel<8, OVERLAP>), grid, block, p.pl.bytes, stream, p);
    else if (p.pl.lanes == 16)
        hipLaunchKernelGGL((explain_kernel<16, OVERLAP>), grid, block, p.pl.bytes, stream, p);
    else
        hipLaunchKernelGGL((explain_kernel<64, OVERLAP>), grid, block, p.pl.bytes, stream, p);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

// pn_explain_groups (M == 0: `group` is [S, W]) and pn_explain_overlap (M >= 1: [S, W, M] labels): the same checks, the same
// route, the same kernel body
int run_explain(const char *who, pn_context *ctx, int64_t S, int32_t W, int32_t H, int32_t C, int32_t G, int32_t M,
                const float *state, int64_t ld_state, const float *coef, const float *ego, int64_t ld_ego, const float *fc2_w,
                int64_t ld_w, const float *fc2_b, const float *weight, const int32_t *group, int32_t norm, int32_t renorm,
                const int64_t *target, const pn_explain_out *out, int32_t *status, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_shape(who, S, W, H, C, G)) return rc;
    if (!out) PN_FAIL(PN_ERR_ARG, "%s: null output description", who);
    if (norm != PN_PATH_NORM_SUM && norm != PN_PATH_NORM_COUNT) PN_FAIL(PN_ERR_ARG, "%s: norm %d", who, norm);
    if (renorm != 0 && renorm != 1) PN_FAIL(PN_ERR_ARG, "%s: renorm %d, 0 or 1", who, renorm);
    if (ld_state < H || ld_ego < H || ld_w < 2 * (int64_t)H)
        PN_FAIL(PN_ERR_ARG, "%s: leading dimensions %lld / %lld / %lld, at least %d / %d / %d", who, (long long)ld_state,
                (long long)ld_ego, (long long)ld_w, H, H, 2 * H);
    if (S > 0 && (!state || !coef || !ego || !fc2_w || !fc2_b || !group))
        PN_FAIL(PN_ERR_ARG, "%s: null state, coef, ego, fc2_w, fc2_b or %s", who, M ? "label" : "group");
    if (int rc = pn::context_check_device(ctx)) return rc;
    if (S == 0) return PN_OK;
    Params p{};
    p.S = S;
    p.W = W;
    p.H = H;
    p.C = C;
    p.G = G;
    p.M = M;
    p.state = state;
    p.ld_state = ld_state;
    p.coef = coef;
    p.ego = ego;
    p.ld_ego = ld_ego;
    p.w = fc2_w;
    p.ld_w = ld_w;
    p.b = fc2_b;
    p.weight = weight;
    p.group = group;
    p.norm = norm;
    p.renorm = renorm;
    p.target = target;
    p.o = *out;
    p.status = status;
    p.pl = plan_of(S, W, H, C, G, M);
    return M ? launch_explain<true>(ctx, p, stream) : launch_explain<false>(ctx, p, stream);
}

}  // namespace

extern "C" {

int pn_explain_route(int64_t S, int32_t W, int32_t H, int32_t C, int32_t G, int32_t route[4]) {
    if (!route) PN_FAIL(PN_ERR_ARG, "pn_explain_route: null result");
    if (int rc = check_shape("pn_explain_route", S, W, H, C, G)) return rc;
    const Plan pl = plan_of(S, W, H, C, G);
    route[0] = pl.route;
    route[1] = pl.lanes;
    route[2] = pl.Cc;
    route[3] = pl.Ht;
    return PN_OK;
}

int pn_explain_groups(pn_context *ctx, int64_t S, int32_t W, int32_t H, int32_t C, int32_t G, const float *state,
                      int64_t ld_state, const float *coef, const float *ego, int64_t ld_ego, const float *fc2_w, int64_t ld_w,
                      const float *fc2_b, const float *weight, const int32_t *group, int32_t norm, int32_t renorm,
                      const int64_t *target, const pn_explain_out *out, int32_t *status, void *stream) {
    return run_explain("pn_explain_groups", ctx, S, W, H, C, G, 0, state, ld_state, coef, ego, ld_ego, fc2_w, ld_w, fc2_b, weight,
                       group, norm, renorm, target, out, status, stream);
}

int pn_explain_overlap(pn_context *ctx, int64_t S, int32_t W, int32_t H, int32_t C, int32_t G, int32_t M, const float *state,
                       int64_t ld_state, const float *coef, const float *ego, int64_t ld_ego, const float *fc2_w, int64_t ld_w,
                       const float *fc2_b, const float *weight, const int32_t *label, int32_t norm, int32_t renorm,
                       const int64_t *target, const pn_explain_out *out, int32_t *status, void *stream) {
    if (M < 1 || M > kMaxM) PN_FAIL(PN_ERR_ARG, "pn_explain_overlap: %d labels per member, 1 .. %d", M, kMaxM);
    if (W >= 1 && (int64_t)W * M > kMaxLabels)
        PN_FAIL(PN_ERR_ARG, "pn_explain_overlap: W * M = %lld labels per row, at most %d", (long long)W * M, kMaxLabels);
    return run_explain("pn_explain_overlap", ctx, S, W, H, C, G, M, state, ld_state, coef, ego, ld_ego, fc2_w, ld_w, fc2_b, weight,
                       label, norm, renorm, target, out, status, stream);
}

int pn_explain_totals(pn_context *ctx, int64_t S, int32_t G, const float *drop_delta, const float *keep_gain,
                      const uint8_t *flip, const int32_t *present, const int32_t *rows, int64_t n_rows, void *totals,
                      void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (S < 0 || S > 2147483647LL) PN_FAIL(PN_ERR_ARG, "pn_explain_totals: %lld rows, 0 .. 2^31 - 1", (long long)S);
    if (G < 1 || G > kMaxG) PN_FAIL(PN_ERR_ARG, "pn_explain_totals: %d groups, 1 .. %d", G, kMaxG);
    if (n_rows < 0 || n_rows > 2147483647LL || (!rows && n_rows != 0))
        PN_FAIL(PN_ERR_ARG, "pn_explain_totals: %lld listed rows%s", (long long)n_rows, rows ? "" : " without a list");
    const int64_t n = rows ? n_rows : S;
    if (n > 0 && S > 0 && (!drop_delta || !keep_gain || !flip || !present || !totals))
        PN_FAIL(PN_ERR_ARG, "pn_explain_totals: null drop_delta, keep_gain, flip, present or totals");
    if (int rc = pn::context_check_device(ctx)) return rc;
    if (n == 0 || S == 0) return PN_OK;
    hipLaunchKernelGGL(explain_totals_kernel, dim3(blocks_for(G)), dim3(kThreads), 0, stream, S, G, drop_delta, keep_gain, flip,
                       present, rows, n, totals);
    PN_CHECK_HIP(hipGetLastError());
    return PN_OK;
}

}  // extern "C"
