// Sorted top-k key lists in registers and the kernels that build and merge them.
#pragma once
#include "engine_prims.h"

namespace range_hip {

// ------------------------------------------------------------------------------------------------
// Top-k lists: 64-bit keys (ordered value bits << 32 | ~row): larger key = larger similarity,
// ties -> lower row index.  (The small-batch HBM-streaming scan that uses them: topk_stream.h.)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long topk_key(float v, uint32_t row) {
    const uint32_t b = __float_as_uint(v);
    const uint32_t o = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((unsigned long long)o << 32) | (unsigned long long)(0xFFFFFFFFu - row);
}
__device__ __forceinline__ float topk_key_val(unsigned long long k) {
    const uint32_t o = (uint32_t)(k >> 32);
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
__device__ __forceinline__ uint32_t topk_key_row(unsigned long long k) { return 0xFFFFFFFFu - (uint32_t)k; }

struct KeyList {                       // sorted descending; 0 = empty slot
    unsigned long long k[MAX_TOPK];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int i = 0; i < MAX_TOPK; ++i) k[i] = 0ull;
    }
    __device__ __forceinline__ void push(unsigned long long x) {
        if (x > k[MAX_TOPK - 1]) {
            k[MAX_TOPK - 1] = x;
#pragma unroll
            for (int i = MAX_TOPK - 1; i > 0; --i) {
                const unsigned long long a = k[i - 1], b = k[i];
                k[i - 1] = a > b ? a : b;
                k[i] = a > b ? b : a;
            }
        }
    }
    __device__ __forceinline__ void pop() {
#pragma unroll
        for (int i = 0; i + 1 < MAX_TOPK; ++i) k[i] = k[i + 1];
        k[MAX_TOPK - 1] = 0ull;
    }
};

// merge the sorted lists held by lanes (j, g=0..3) of one query j: afterwards every such lane
// holds the same top-MAX_TOPK list.  Keys are unique (the row is part of the key).
__device__ __forceinline__ void merge_lane_groups(KeyList& L) {
    KeyList R;
#pragma unroll
    for (int i = 0; i < MAX_TOPK; ++i) {
        const unsigned long long h = L.k[0];
        unsigned long long m = h;
        unsigned long long o = lane_xor_u64<16>(m); m = o > m ? o : m;
        o = lane_xor_u64<32>(m); m = o > m ? o : m;
        R.k[i] = m;
        if (h == m && m != 0ull) L.pop();
    }
    L = R;
}

// top list of the 64 sorted lists held by the lanes of one wave (no barrier: shuffles only)
__device__ __forceinline__ void merge_wave(KeyList& L) {
    KeyList R;
#pragma unroll
    for (int i = 0; i < MAX_TOPK; ++i) {
        const unsigned long long h = L.k[0];
        unsigned long long m = h;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long o = shfl_xor_u64(m, off);
            m = o > m ? o : m;
        }
        R.k[i] = m;
        if (h == m && m != 0ull) L.pop();
    }
    L = R;
}

// theta[q] = the 16th largest of the n_parts*4 per-lane-group maxima pass 1 recorded for query q
// (-inf when there are fewer than 16): a lower bound of the query's 16th best similarity, and a
// tight one - with 52 groups about 20 of 100 000 values reach it.  One wave per query.
__global__ __launch_bounds__(256) void topk_threshold_kernel(const float* __restrict__ rowmax,
                                                             int n_parts, int64_t B,
                                                             float* __restrict__ theta) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= B) return;
    KeyList L;
    L.init();
    const int total = n_parts * 4;
    for (int e = lane; e < total; e += 64) {
        const float v = rowmax[((int64_t)(e >> 2) * B + q) * 4 + (e & 3)];
        if (v > -INFINITY) L.push(topk_key(v, (uint32_t)e));
    }
    merge_wave(L);
    if (lane == 0) theta[q] = L.k[MAX_TOPK - 1] ? topk_key_val(L.k[MAX_TOPK - 1]) : -INFINITY;
}

// Top-k from the KEPT logits (large batches): the semantic similarities of pass 1 are already in
// HBM, one 1 KB tile per (query tile, 16-row block, wave slot); this kernel streams them back
// (HBM-bound: 4 B per (query,row) pair) and keeps a running top-16 per lane.  A lane sees thousands
// of values here, so its list saturates and nearly every value fails the first comparison -
// unlike inside pass 1, where the list maintenance of the TOPK variant costs more than the MFMAs.
// One wave per (wave slot of 16 queries, chunk of blocks); lane (j,g) reads the float4 of rows
// pi_row(4g+r); the 4 lane groups of a query are merged and one sorted list of 16 (value, local
// row) goes to cval/cidx[(chunk*B + query)*16 ...], merged across chunks by merge_topk_wave_kernel.
__global__ __launch_bounds__(256) void topk_from_logits_kernel(const float* __restrict__ logits,
                                                               int32_t n_blocks, int64_t B,
                                                               int64_t n_valid, int32_t n_chunks,
                                                               const float* __restrict__ theta,
                                                               float* __restrict__ cval,
                                                               int32_t* __restrict__ cidx) {
    const int lane = threadIdx.x & 63, g = lane >> 4;
    const int64_t slot = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // (query tile, wave)
    const int64_t n_slots = (B + 15) / 16;
    if (slot >= n_slots) return;
    const int chunk = blockIdx.y;
    const int b0 = part_begin(chunk, n_blocks, n_chunks);
    const int b1 = part_begin(chunk + 1, n_blocks, n_chunks);
    // tile (qtile, b, wave) sits at ((qtile * n_blocks + b) * 4 + wave) * 256 floats
    const float* base = logits + ((slot >> 2) * (int64_t)n_blocks * 4 + (slot & 3)) * 256 + 4 * lane;
    int prow[4];
    lane_rows(prow, g);
    KeyList L;
    L.init();
    // lower bound of this lane's query's 16th best similarity (topk_threshold_kernel): only the
    // few values that reach it are candidates, so the (wave-divergent) insertion is rare
    const int64_t qq = slot * 16 + (lane & 15);
    const float th = theta[qq < B ? qq : B - 1];
    constexpr int UNROLL = 8;
    for (int b = b0; b < b1; b += UNROLL) {
        f32x4 v[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int bb = b + u < b1 ? b + u : b1 - 1;
            v[u] = *reinterpret_cast<const f32x4*>(base + (int64_t)bb * 1024);
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            if (b + u < b1) {
                const int64_t row0 = (int64_t)(b + u) * BLK;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t row = row0 + prow[r];
                    if (v[u][r] >= th && row < n_valid) L.push(topk_key(v[u][r], (uint32_t)row));
                }
            }
        }
    }
    merge_lane_groups(L);
    const int64_t q = slot * 16 + (lane & 15);
    if (g == 0 && q < B) {
        float* ov = cval + ((int64_t)chunk * B + q) * MAX_TOPK;
        int32_t* oi = cidx + ((int64_t)chunk * B + q) * MAX_TOPK;
#pragma unroll
        for (int i = 0; i < MAX_TOPK; ++i) {
            const unsigned long long mm = L.k[i];
            ov[i] = mm ? topk_key_val(mm) : -INFINITY;
            oi[i] = mm ? (int32_t)topk_key_row(mm) : 0x7fffffff;
        }
    }
}

// Top-k of the pass-1 candidates of one query (scan_stats_kernel<.., true>): one WAVE per query.
// cval / cidx: (n_parts, B, per_part) sorted-by-lane-group candidate values and LOCAL rows
// (0x7fffffff = empty).  Lane l folds candidates l, l+64, ... into a register list, the wave then
// extracts the k best (ties -> lower row) by shuffles.
__global__ __launch_bounds__(256) void merge_topk_wave_kernel(const float* __restrict__ cval,
                                                              const int32_t* __restrict__ cidx,
                                                              int n_parts, int64_t B, int per_part,
                                                              int k, int64_t row_offset,
                                                              float* __restrict__ oval,
                                                              int64_t* __restrict__ oidx) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= B) return;
    KeyList L;
    L.init();
    const int total = n_parts * per_part;
    for (int e = lane; e < total; e += 64) {
        const int p = e / per_part, c = e - p * per_part;
        const int64_t at = ((int64_t)p * B + q) * per_part + c;
        const int32_t row = cidx[at];
        if (row != 0x7fffffff) L.push(topk_key(cval[at], (uint32_t)row));
    }
    merge_wave(L);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < MAX_TOPK; ++i) {
            if (i < k) {
                const unsigned long long mm = L.k[i];
                oval[q * k + i] = mm ? topk_key_val(mm) : -INFINITY;
                oidx[q * k + i] = mm ? (int64_t)topk_key_row(mm) + row_offset : (int64_t)-1;
            }
        }
    }
}

}  // namespace range_hip
