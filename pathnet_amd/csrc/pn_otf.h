// pn_otf.h -- device helpers of the on-the-fly hop codes, shared by the walker (pn_sampler.hip) and the path annotator
// (pn_codes.hip): the per-wave LDS hash table that holds the out-ball of a source node with exact distances, and the
// Bloom filter over the out-neighbours of the ball's outermost level.  Why the ball and a bounded search over
// in-neighbour chains give exact hop counts: the comment above merw_walk_otf_kernel.
// Also the two table look-ups that the biased walker (pn_bias.hip) and its likelihood (pn_prob.hip) must agree on:
// node_table and has_edge.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

// the table of node x: its first triple and its length, from node_ref ({first triple, count}: one 8-byte load) or, when
// that is null, from two words of off[]
__device__ __forceinline__ void node_table(const uint2 *node_ref, const int64_t *off, int32_t x, int64_t &o0, int32_t &len) {
    if (node_ref) {
        const uint2 r = node_ref[x];
        o0 = r.x;
        len = (int32_t)r.y;
    } else {
        o0 = off[x];
        len = (int32_t)(off[x + 1] - o0);
    }
}

// the directed edge a -> b (a != b) in the hop source: one byte of the dense table, or (dis == null) a binary search of
// a's sorted out-list
__device__ __forceinline__ bool has_edge(const uint8_t *dis, const int64_t *adj_off, const int32_t *adj, int32_t n, int32_t a,
                                         int32_t b) {
    if (dis) return dis[(size_t)a * (size_t)n + (size_t)b] == 2;
    int64_t lo = adj_off[a], hi = adj_off[a + 1];
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int32_t v = adj[mid];
        if (v == b) return true;
        if (v < b)
            lo = mid + 1;
        else
            hi = mid;
    }
    return false;
}

constexpr int kOtfWaves = 2;                  // source nodes per workgroup (16 KB of LDS each; a workgroup's 32 KB plus its
                                              // few counter words let four workgroups share a CU's 160 KiB)
constexpr int kOtfCap = 2048;                 // hash slots per wave (8 KB)
constexpr uint32_t kOtfEmpty = 0xFFFFFFFFu;
constexpr int kOtfMaxDepth = 8;
constexpr int kOtfBloomWords = 1024;          // 32 Kbit per wave
__device__ __forceinline__ void otf_bloom_bits(int32_t node, uint32_t &b0, uint32_t &b1, uint32_t &b2) {
    b0 = ((uint32_t)node * 0x9E3779B1u) >> 17;         // 15 bits each
    b1 = ((uint32_t)node * 0x85EBCA6Bu + 0x27D4EB2Fu) >> 17;
    b2 = ((uint32_t)node * 0xC2B2AE35u + 0x165667B1u) >> 17;
}
__device__ __forceinline__ bool otf_bloom_maybe(const uint32_t *bloom, int32_t node) {
    uint32_t b0, b1, b2;
    otf_bloom_bits(node, b0, b1, b2);
    return ((bloom[b0 >> 5] >> (b0 & 31)) & (bloom[b1 >> 5] >> (b1 & 31)) & (bloom[b2 >> 5] >> (b2 & 31)) & 1u) != 0;
}

__device__ __forceinline__ uint32_t otf_hash(uint32_t x) {
    x *= 0x9E3779B1u;
    return (x ^ (x >> 15)) & (kOtfCap - 1);
}
// returns true if (node, d) was newly inserted
__device__ __forceinline__ bool otf_insert(uint32_t *tab, int32_t node, int d) {
    uint32_t h = otf_hash((uint32_t)node);
    const uint32_t packed = ((uint32_t)node << 3) | (uint32_t)d;
    for (int probe = 0; probe < kOtfCap; probe++) {
        const uint32_t old = atomicCAS(&tab[h], kOtfEmpty, packed);
        if (old == kOtfEmpty) return true;
        if ((old >> 3) == (uint32_t)node) return false;     // already there with a level <= d
        h = (h + 1) & (kOtfCap - 1);
    }
    return false;
}
__device__ __forceinline__ int otf_lookup(const uint32_t *tab, int32_t node) {
    uint32_t h = otf_hash((uint32_t)node);
    for (int probe = 0; probe < kOtfCap; probe++) {
        const uint32_t v = tab[h];
        if (v == kOtfEmpty) return -1;
        if ((v >> 3) == (uint32_t)node) return (int)(v & 7u);
        h = (h + 1) & (kOtfCap - 1);
    }
    return -1;
}


// Out-ball of st in the wave's table: the largest radius of 2, 1, 0 that keeps the table at most half full, with exact
// distances (level-synchronous, insert-if-absent keeps the smaller level).  The ball of the returned radius is complete.
// Wave-uniform; cnt is the wave's counter word in LDS (left holding the number of ball nodes).
__device__ __forceinline__ int otf_build_ball(uint32_t *tab, int *cnt, const int lane, const int32_t st,
                                              const int64_t *__restrict__ adj_off, const int32_t *__restrict__ adj) {
    int rf = 2;
    for (;; rf--) {
        for (int i = lane; i < kOtfCap; i += 64) tab[i] = kOtfEmpty;
        if (lane == 0) *cnt = 0;
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
            otf_insert(tab, st, 0);
            *cnt = 1;
        }
        __builtin_amdgcn_wave_barrier();
        const int64_t b0 = adj_off[st], e0 = adj_off[st + 1];
        bool overflow = false;
        if (rf >= 1) {
            if (e0 - b0 > kOtfCap / 2) overflow = true;
            if (!overflow) {
                for (int64_t j = b0 + lane; j < e0; j += 64)
                    if (otf_insert(tab, adj[j], 1)) atomicAdd(cnt, 1);
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (rf >= 2 && !overflow) {
            for (int64_t j = b0; j < e0 && !overflow; j++) {
                const int32_t a = adj[j];
                const int64_t b1 = adj_off[a], e1 = adj_off[a + 1];
                if (*cnt + (e1 - b1) > kOtfCap / 2) {    // could exceed half load: give up this radius
                    overflow = true;
                    break;
                }
                for (int64_t k = b1 + lane; k < e1; k += 64)
                    if (otf_insert(tab, adj[k], 2)) atomicAdd(cnt, 1);
                __builtin_amdgcn_wave_barrier();
            }
        }
        if (!overflow || rf == 0) break;
    }
    __builtin_amdgcn_wave_barrier();
    return rf;
}

// The out-neighbours of the ball's nodes of level `level` -> Bloom filter (three bits each; no false negatives).
// list: kOtfCap / 2 words of the wave's LDS (the table is at most half full).  Wave-uniform.
__device__ __forceinline__ void otf_build_bloom(uint32_t *bloom, const uint32_t *tab, int *cnt, uint32_t *list,
                                                const int lane, const uint32_t level,
                                                const int64_t *__restrict__ adj_off, const int32_t *__restrict__ adj) {
    for (int i = lane; i < kOtfBloomWords; i += 64) bloom[i] = 0u;
    if (lane == 0) *cnt = 0;
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < kOtfCap; i += 64) {
        const uint32_t v = tab[i];
        if (v != kOtfEmpty && (v & 7u) == level) list[atomicAdd(cnt, 1)] = v >> 3;
    }
    __builtin_amdgcn_wave_barrier();
    const int n2 = *cnt;
    // a lane per listed node: its out-neighbours, three bits each; the list bounds of a lane's NEXT node are fetched
    // while it walks the current one
    int64_t kb_n = 0, ke_n = 0;
    if (lane < n2) kb_n = adj_off[(int32_t)list[lane]], ke_n = adj_off[(int32_t)list[lane] + 1];
    for (int i = lane; i < n2; i += 64) {
        const int64_t kb = kb_n, ke = ke_n;
        if (i + 64 < n2) kb_n = adj_off[(int32_t)list[i + 64]], ke_n = adj_off[(int32_t)list[i + 64] + 1];
        for (int64_t k = kb; k < ke; k += 4) {       // four loads in flight (the tail repeats the last entry)
            int32_t nb[4];
#pragma unroll
            for (int u = 0; u < 4; u++) nb[u] = adj[min(k + u, ke - 1)];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                uint32_t b0, b1, b2;
                otf_bloom_bits(nb[u], b0, b1, b2);
                atomicOr(&bloom[b0 >> 5], 1u << (b0 & 31));
                atomicOr(&bloom[b1 >> 5], 1u << (b1 & 31));
                atomicOr(&bloom[b2 >> 5], 1u << (b2 & 31));
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
}

}  // namespace
