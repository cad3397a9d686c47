// pn_pool_step2.inc -- pool_step2_kernel, the fused pooling step with the node's rows in registers (pn_pool.hip includes this
// text twice).  Plain, it is pool_step2_kernel exactly as it stood in pn_pagg.hip; with PN_STEP2_LOSS_OPTS defined it is
// pool_step2_loss_kernel, the same kernel with pn_loss_spec's options in its cross-entropy block.  The preprocessor and not
// a template parameter: the plain kernel's text is then token for token what it was, and so is its code (as a template
// over the options the same lines got another scalar register allocation).
template <int MM, int HI>
#ifdef PN_STEP2_LOSS_OPTS
__global__ __launch_bounds__(256, 6) void pool_step2_loss_kernel(PoolStepLossParams q) {
    const PoolStepParams &p = q.s;
    const LossOpts &o = q.o;
#else
__global__ __launch_bounds__(256, 6) void pool_step2_kernel(PoolStepParams p) {      // (six workgroups per CU: 1 536 slots)
#endif
    extern __shared__ float lds[];
    const PoolParams &f = p.f;
    const PoolBwdParams &b = p.b;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int g = blockIdx.x, H = f.H, W = f.W, C = f.C;
    const bool has_att = f.variant != PN_VARIANT_PAGG;
    // per-member scalars (wave-uniform) live in LDS, [wave][MM] each: as register arrays they cost 40 VGPRs and two of the six
    // workgroups a CU can hold
    float *cf = lds + wave * MM;        // [4][MM] pooling coefficients
    float *dsl = lds + 4 * MM + wave * MM;      // [4][MM] d score
    float *sc = lds + 8 * MM;           // [4 MM] activated scores in member order (HETERO softmax)
    float *part4 = sc + 4 * MM;         // [4][H]  waves' partial pooled sums; later [4][2H] attention-weight partials
    float *l1s = part4 + 8 * H;         // [2H] classifier input
    float *dp = l1s + 2 * H;            // [H]  d pooled / W
    float *lg = dp + H;                 // [C] logits, then [C] their gradient
    float *s_tot = lg + 2 * C;          // [4]
    const float inv_w = 1.0f / (float)W;
    const int64_t s0 = (int64_t)g * W;
    PTRACE(0);

    // ---- everything the node needs from memory, requested at once
    float hn[MM][HI], e_r[HI], aw_h[HI], aw_e[HI];
    const int e0 = has_att ? f.egoidx[s0] : 0;
    // (the node's own row of Xh, its target and the attention weights are asked for here as well, with the rows: loaded where they
    //  are used they were two more dependent round trips behind barriers)
    const int sel_g = min(max(f.sel[g], 0), f.N - 1);
    // (a target outside [0, C): NaN loss, zero gradient row; the index into lg[] is clamped -- selects, no branch, no address
    //  formed from it.  Workgroup-uniform: scalar registers)
    const int64_t tgt64 = p.target[g];
    const bool tgt_ok = tgt64 >= 0 && tgt64 < (int64_t)C;
    const int tgt = tgt_ok ? (int)tgt64 : 0;
#ifdef PN_STEP2_LOSS_OPTS
    // (the target's class weight and the denominator travel with the loads here, not behind the logits' barrier)
    float k_grad, k_loss;
    loss_factors(o, k_grad, k_loss);
    const bool tgt_ign = o.has_ignore && tgt64 == o.ignore;
    const float tgt_a = (1.0f - o.eps) * (o.weight ? o.weight[tgt] : 1.0f);
#endif
    int same = 1;
    const float *hn_g = f.hn + s0 * H;          // (a scalar base + one 32-bit offset per load: twenty 64-bit addresses would not fit)
    // Every load below is unconditional (clamped addresses) and its value always used -- rows past W / columns past H are zeroed by a
    // MULTIPLICATION, the members' start rows compared whatever the variant (PAGG: a valid dummy).  As selects, hipcc moved each load
    // into a branch of its own with a wait behind it: thirty dependent round trips, 18 of the kernel's 40 us (r06_glue.txt section 23).
    const int32_t *ego_g = has_att ? f.egoidx + s0 : reinterpret_cast<const int32_t *>(hn_g);
    int egv[MM];
#pragma unroll
    for (int k = 0; k < MM; k++) {
        const uint32_t memc = (uint32_t)min(wave + 4 * k, W - 1);
        egv[k] = ego_g[memc];
#pragma unroll
        for (int i = 0; i < HI; i++) hn[k][i] = hn_g[memc * (uint32_t)H + (uint32_t)min(lane + 64 * i, H - 1)];
    }
#pragma unroll
    for (int k = 0; k < MM; k++) {
        same &= (int)(egv[k] == e0) | (int)!has_att;
#pragma unroll
        for (int i = 0; i < HI; i++) hn[k][i] *= (wave + 4 * k < W && lane + 64 * i < H) ? 1.0f : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < HI; i++) {
        const int j = lane + 64 * i, jc = min(j, H - 1);
        aw_h[i] = (has_att && j < H) ? f.att_w[jc] : 0.0f;
        aw_e[i] = (has_att && j < H) ? f.att_w[H + jc] : 0.0f;
        e_r[i] = (has_att && j < H) ? f.ego_tab[(int64_t)e0 * H + jc] : 0.0f;
    }
    const float xh_own = f.Xh[(int64_t)sel_g * H + min(tid, H - 1)];
    const bool one_row = __syncthreads_and(same) != 0;
    PTRACE(1);
    // ---- scores and pooling coefficients of this wave's members (raw scores -> cf[], LeakyReLU slopes -> bits of `neg`)
    uint32_t neg = 0;       // bit k: member k's raw score <= 0
    if (has_att) {
        const float ab = f.att_b[0];
        float edot = 0.0f;
#pragma unroll
        for (int i = 0; i < HI; i++) edot += e_r[i] * aw_e[i];
        edot = wave_sum_u(edot);
#pragma unroll
        for (int k = 0; k < MM; k++) {
            const int mem = wave + 4 * k;
            float part = 0.0f;
#pragma unroll
            for (int i = 0; i < HI; i++) part += hn[k][i] * aw_h[i];
            float ed = edot;
            if (!one_row) {         // (rare: a member whose path starts elsewhere)
                const int64_t er = (int64_t)f.egoidx[s0 + min(mem, W - 1)] * H;
                float pe = 0.0f;
#pragma unroll
                for (int i = 0; i < HI; i++) {
                    const int j = lane + 64 * i;
                    if (j < H) pe += f.ego_tab[er + j] * aw_e[i];
                }
                ed = wave_sum_u(pe);
            }
            const float raw = wave_sum_u(part) + ed + ab;
            if (!(raw > 0.0f)) neg |= 1u << k;
            if (lane == 0) {
                cf[k] = raw;
                if (mem < W) f.rawsc[s0 + mem] = raw;
            }
        }
    } else if (lane == 0) {
#pragma unroll
        for (int k = 0; k < MM; k++) {
            cf[k] = 0.0f;
            if (wave + 4 * k < W) f.rawsc[s0 + wave + 4 * k] = 0.0f;
        }
    }
    if (f.variant == PN_VARIANT_HETERO) {       // softmax over the W members of LeakyReLU(score)
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < MM; k++) {
                const int mem = wave + 4 * k;
                const float r = cf[k];
                if (mem < W) sc[mem] = r > 0.0f ? r : 0.01f * r;
            }
        }
        __syncthreads();
        const float v = lane < W ? sc[lane] : -3.4e38f;       // (W <= 4 MM <= 64)
        const float mx = wave_max(v);
        const float sum = wave_sum_u(lane < W ? expf(v - mx) : 0.0f);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < MM; k++) {
                const float r = cf[k];
                cf[k] = expf((r > 0.0f ? r : 0.01f * r) - mx) / sum;
            }
        }
    } else if (lane == 0) {
#pragma unroll
        for (int k = 0; k < MM; k++) cf[k] = f.variant == PN_VARIANT_HOMO ? 1.0f + cf[k] : 1.0f;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // (cf[] of this wave: written by lane 0, read by the wave)
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < MM; k++)
            if (wave + 4 * k < W) f.coef[s0 + wave + 4 * k] = cf[k];
    }
    // ---- pooled = mean_w coef_w h_w
    PTRACE(2);
#pragma unroll
    for (int i = 0; i < HI; i++) {
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < MM; k++) acc += cf[k] * hn[k][i];       // (members past W hold zeros)
        const int j = lane + 64 * i;
        if (j < H) part4[wave * H + j] = acc;
    }
    __syncthreads();
    PTRACE(3);
    // ---- layer1 = dropout([Xh[sel[g]] ; pooled]); the masks stay in registers for the backward
    float m_a = 1.0f, m_b = 1.0f;       // this thread's column tid (< H)
    if (tid < H) {
        const int j = tid;
        const uint64_t gg = (uint64_t)(f.goff + g);
        float a = xh_own, bq = (part4[j] + part4[H + j] + part4[2 * H + j] + part4[3 * H + j]) * inv_w;
        if (f.mask) {
            m_a = f.mask[gg * 2 * H + j];
            m_b = f.mask[gg * 2 * H + H + j];
        } else if (f.p_drop > 0.0f) {
            const uint64_t seed = f.dyn ? f.dyn->seed : f.seed;
            m_a = dropout1(seed, gg * 2 * H + j, 2u, f.p_drop);
            m_b = dropout1(seed, gg * 2 * H + H + j, 2u, f.p_drop);
        }
        a *= m_a;
        bq *= m_b;
        float *l1 = f.layer1 + (int64_t)g * 2 * H;
        l1[j] = a;
        l1[H + j] = bq;
        l1s[j] = a;
        l1s[H + j] = bq;
    }
    __syncthreads();
    PTRACE(4);
    for (int c = wave; c < C; c += 4) {
        // (a fixed trip count with clamped addresses: the row's loads leave together instead of one round trip per 64 columns)
        const float *wrow = f.fc2_w + (int64_t)c * 2 * H;
        float wv[2 * HI];
#pragma unroll
        for (int q = 0; q < 2 * HI; q++) wv[q] = wrow[min(lane + 64 * q, 2 * H - 1)];
        float part = 0.0f;
#pragma unroll
        for (int q = 0; q < 2 * HI; q++) {
            const int j = lane + 64 * q;
            if (j < 2 * H) part += l1s[j] * wv[q];
        }
        part = wave_sum_u(part);
        if (lane == 0) {
            const float v = part + f.fc2_b[c];
            f.out[(int64_t)g * C + c] = v;
            lg[c] = v;
        }
    }
    __syncthreads();
    PTRACE(5);
    if (wave == 0) {        // the row's cross entropy as cross_entropy_kernel computes it, a lane per class (the sum in another order)
        float m = -3.4e38f;
        for (int c = lane; c < C; c += 64) m = fmaxf(m, lg[c]);
        m = wave_max(m);
        float sum = 0.0f;
        for (int c = lane; c < C; c += 64) sum += expf(lg[c] - m);
        const float ls = logf(wave_sum_u(sum));
        const int t = tgt;
#ifdef PN_STEP2_LOSS_OPTS
        // pn_loss.h's row with a lane per class: smoothing adds one wave sum of w[c] lp[c] (and one of w[c])
        const bool kept = tgt_ok && !tgt_ign, smooth = o.eps != 0.0f;
        const float es = o.eps / (float)C;
        float row = tgt_a * (ls - (lg[t] - m)), wsum = 0.0f;
        if (smooth) {       // (workgroup-uniform)
            float sm = 0.0f;
            for (int c = lane; c < C; c += 64) {
                const float wc = o.weight ? o.weight[c] : 1.0f;
                sm += wc * (ls - (lg[c] - m));
                wsum += wc;
            }
            sm = wave_sum_u(sm);
            wsum = wave_sum_u(wsum);
            row += es * sm;
        }
        if (lane == 0) p.lossg[g] = tgt_ign ? 0.0f : (tgt_ok ? row : NAN);
        float *go = p.gout + (int64_t)g * C;
        for (int c = lane; c < C; c += 64) {
            const float pc = expf((lg[c] - m) - ls);
            float gv = ((pc - (c == t ? 1.0f : 0.0f)) * tgt_a) * k_grad;
            if (smooth) gv += (es * (wsum * pc - (o.weight ? o.weight[c] : 1.0f))) * k_grad;
            go[c] = kept ? gv : 0.0f;
            lg[C + c] = kept ? gv : 0.0f;
        }
#else
        const float row = ls - (lg[t] - m);
        if (lane == 0) p.lossg[g] = tgt_ok ? row : NAN;
        float *go = p.gout + (int64_t)g * C;
        for (int c = lane; c < C; c += 64) {
            const float gv = (expf((lg[c] - m) - ls) - (c == t ? 1.0f : 0.0f)) * p.scale;
            go[c] = tgt_ok ? gv : 0.0f;
            lg[C + c] = tgt_ok ? gv : 0.0f;
        }
#endif
    }
    __syncthreads();
    PTRACE(6);
    // ---- backward: d layer1 = g_out . fc2_w (masked): its ego half onto the node's row of d Xh, its pooled half / W = dp
    if (tid < H) {
        const int j = tid;
        float a = 0.0f, bq = 0.0f;
        for (int c0 = 0; c0 < C; c0 += 4) {     // four classes' loads in flight (clamped rows, masked sums)
            float wa[4], wb[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float *wrow = f.fc2_w + (int64_t)min(c0 + q, C - 1) * 2 * H;
                wa[q] = wrow[j];
                wb[q] = wrow[H + j];
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float go = c0 + q < C ? lg[C + c0 + q] : 0.0f;
                a += go * wa[q];
                bq += go * wb[q];
            }
        }
        atomicAdd(&b.dXh[(int64_t)sel_g * H + j], a * m_a);
        dp[j] = bq * m_b * inv_w;
    }
    __syncthreads();
    PTRACE(7);
    float dpr[HI];
#pragma unroll
    for (int i = 0; i < HI; i++) {
        const int j = lane + 64 * i;
        dpr[i] = j < H ? dp[j] : 0.0f;
    }
    {       // d coef of this wave's members -> dsl[]; HETERO: through the softmax
        float tpart = 0.0f;
#pragma unroll
        for (int k = 0; k < MM; k++) {
            float part = 0.0f;
#pragma unroll
            for (int i = 0; i < HI; i++) part += hn[k][i] * dpr[i];
            const float dco = wave_sum_u(part);
            if (wave + 4 * k < W) tpart += cf[k] * dco;
            if (lane == 0) dsl[k] = dco;
        }
        if (f.variant == PN_VARIANT_HETERO) {
            if (lane == 0) s_tot[wave] = tpart;
            __syncthreads();
            const float tot = (s_tot[0] + s_tot[1]) + (s_tot[2] + s_tot[3]);
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < MM; k++) dsl[k] = cf[k] * (dsl[k] - tot) * ((neg >> k) & 1u ? 0.01f : 1.0f);
            }
        } else if (f.variant != PN_VARIANT_HOMO && lane == 0) {
#pragma unroll
            for (int k = 0; k < MM; k++) dsl[k] = 0.0f;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    PTRACE(8);
    // ---- per member: d h_n; the attention-weight and attention-ego terms accumulate in registers
    float gaw_h[HI], gaw_e[HI], ego_acc[HI], gab = 0.0f;
#pragma unroll
    for (int i = 0; i < HI; i++) gaw_h[i] = gaw_e[i] = ego_acc[i] = 0.0f;
#pragma unroll
    for (int k = 0; k < MM; k++) {
        const int mem = wave + 4 * k;
        if (mem >= W) break;            // (wave-uniform)
        const float ds = dsl[k], ck = cf[k];
        const int64_t er = (has_att && !one_row) ? (int64_t)f.egoidx[s0 + mem] * H : 0;
#pragma unroll
        for (int i = 0; i < HI; i++) {
            const int j = lane + 64 * i;
            if (j < H) {
                float dh = ck * dpr[i];
                if (has_att) {
                    dh += ds * aw_h[i];
                    gaw_h[i] += ds * hn[k][i];
                    const float eg = ds * aw_e[i];
                    if (one_row) {
                        gaw_e[i] += ds * e_r[i];
                        ego_acc[i] += eg;
                    } else {
                        gaw_e[i] += ds * f.ego_tab[er + j];
                        atomicAdd(&b.dego[er + j], eg);
                    }
                }
                b.dhn[(s0 + mem) * H + j] = dh;
            }
        }
        gab += ds;
    }
    PTRACE(9);
    if (!has_att) return;       // block-uniform
    float *red = part4;         // [4][2H]
    if (one_row) {
#pragma unroll
        for (int i = 0; i < HI; i++) {
            const int j = lane + 64 * i;
            if (j < H) red[wave * H + j] = ego_acc[i];
        }
        __syncthreads();
        if (tid < H) atomicAdd(&b.dego[(int64_t)e0 * H + tid], (red[tid] + red[H + tid]) + (red[2 * H + tid] + red[3 * H + tid]));
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < HI; i++) {
        const int j = lane + 64 * i;
        if (j < H) {
            red[wave * 2 * H + j] = gaw_h[i];
            red[wave * 2 * H + H + j] = gaw_e[i];
        }
    }
    __syncthreads();
    float *out = b.det_att + (int64_t)g * (2 * H + 4);
    for (int j = tid; j < 2 * H; j += 256) out[j] = red[j] + red[2 * H + j] + red[4 * H + j] + red[6 * H + j];
    if (lane == 0) out[2 * H + wave] = gab;
    PTRACE(10);
}
