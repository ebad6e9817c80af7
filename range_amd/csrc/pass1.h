// Pass 1 of the two-pass soft attention (overview: scan_common.h): the softmax statistics of both
// logit rows, optionally the kept logits and top-k candidates, and the merges of the per-split parts.
#pragma once
#include <type_traits>

#include "scan_common.h"

namespace range_hip {

template <int K>
struct TopK {
    float v[K];
    int32_t i[K];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int k = 0; k < K; ++k) { v[k] = -INFINITY; i[k] = 0x7fffffff; }
    }
    // strict '>' keeps the earlier (lower) row among equal values: a lane meets rows in
    // increasing order.
    __device__ __forceinline__ void push(float x, int32_t idx) {
        if (x > v[K - 1]) {
            v[K - 1] = x; i[K - 1] = idx;
#pragma unroll
            for (int k = K - 1; k > 0; --k) {
                if (v[k] > v[k - 1]) {
                    const float tv = v[k]; v[k] = v[k - 1]; v[k - 1] = tv;
                    const int32_t ti = i[k]; i[k] = i[k - 1]; i[k - 1] = ti;
                }
            }
        }
    }
};

template <bool GEO, bool TOPK>
__global__ __launch_bounds__(256) void scan_stats_kernel(ScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // LDS: K ring 2 x [16][256] f32 | X ring 2 x [16][4] f32 (33 KB: four workgroups per CU)
    const uint32_t lds0 = (uint32_t)(uintptr_t)RANGE_LPTR(smem);
    const uint32_t kring_lds = lds0, xring_lds = lds0 + 2 * BLK * KEY_DIM * 4;
    constexpr uint32_t KT_BYTES = BLK * KEY_DIM * 4;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4;
    const int swz = lane ^ (4 * wave);
    int split, qt;
    decode_block(a, split, qt);
    const int b0 = part_begin(split, a.n_blocks, a.n_splits);
    const int b1 = part_begin(split + 1, a.n_blocks, a.n_splits);
    const int nb = b1 - b0;
    const int64_t q = (int64_t)qt * QTILE + wave * 16 + (lane & 15);

    QFrag f;
    load_qfrag(f, a.ehat, a.xq, a.B, q, g);
    pin_qfrag(f);
    KAddr kaddr;
    kaddr.init(lane);

    // Softmax statistics with a CONSTANT shift.  Both logit rows are dot products of unit vectors
    // (range.py:212 normalises e-hat, :85-89 the keys; utils.py:11-16 gives unit xyz), so
    // t = k * s <= k: the shift m = k (tau * log2 e: 17.3 / 21.6 / 57.7) replaces the running
    // maximum of an online softmax.  2^(t - m) then lies in [2^-2k, 1] - at least 2^-116, a normal
    // float32, for tau <= 43 (checked on the host) - so the statistic of an element is one fma,
    // one exp2 and one add, there is no rescaling, and the statistics of lanes, splits and bank
    // shards merge by plain sums.  Floating point keeps the relative precision of the sum whatever
    // the shift.
    float l1 = 0.f, l2 = 0.f;
    const float nm1 = -a.k_sem, nm2 = -a.k_geo;
    float smax = -INFINITY;      // largest similarity of this lane's rows (a.rowmax)
    TopK<TOPK ? MAX_TOPK : 1> tk;
    if (TOPK) tk.init();

    // ring of 2 K tiles: tile t+1 is requested right after barrier t (every wave is then done
    // with tile t-1, whose slot it re-uses) and waited for before barrier t+1.
    if (nb > 0) {
        issue_k_tile(a.keys, a.xyz4, (int64_t)b0 * BLK, kring_lds, xring_lds, wave, lane, swz);
    }
    int slot = 0;
    for (int t = 0; t < nb; ++t) {
        RANGE_WAIT_BARRIER(0);
        if (t + 1 < nb) {
            const int s2 = slot ^ 1;
            issue_k_tile(a.keys, a.xyz4, (int64_t)(b0 + t + 1) * BLK, kring_lds + s2 * KT_BYTES,
                         xring_lds + s2 * 256, wave, lane, swz);
        }
        QKAcc c;
        qk_mfma<GEO>(smem + slot * KT_BYTES,
                     qk_first_reads<GEO>(smem + slot * KT_BYTES, smem + 2 * KT_BYTES + slot * 256, kaddr),
                     kaddr, f, c, [](int) __attribute__((always_inline)) {});
        c.fence();
        const f32x4 ss = {c.sem(0), c.sem(1), c.sem(2), c.sem(3)};
        const f32x4 sg = c.g;
        if (a.logits)   // keep the tile for pass 2 (the barrier's vmcnt(0) also covers this store)
            // (non-temporal: 4 GB per 10^4 x 10^5 launch that nobody reads before pass 2 - measured
            // three A/B pairs, 10 000 queries: pass 1 3.937 -> 3.916 ms, the pass 2 behind it 14.690 ->
            // 14.616 ms)
            __builtin_nontemporal_store(ss, reinterpret_cast<f32x4*>(a.logits + logit_tile((int64_t)qt + a.qt_offset, a.n_blocks, b0 + t, wave) + 4 * lane));
        // statistics of this tile.  Only the bank's last block can hold pad rows: every other
        // tile takes the unmasked form
        const int64_t row0 = (int64_t)(b0 + t) * BLK;
        const int n_here = (int)(a.n_valid - row0 < BLK ? a.n_valid - row0 : BLK);   // valid rows
        auto tile_stats = [&](auto masked_tag) __attribute__((always_inline)) {
            constexpr bool MASKED = decltype(masked_tag)::value;
            bool ok[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int pr = pi_row(4 * g + r);
                ok[r] = !MASKED || pr < n_here;
                if (TOPK) { if (ok[r]) tk.push(ss[r], (int32_t)(row0 + pr)); }
            }
            if (a.rowmax)
                smax = fmaxf(smax, fmaxf(fmaxf(ok[0] ? ss[0] : -INFINITY, ok[1] ? ss[1] : -INFINITY),
                                         fmaxf(ok[2] ? ss[2] : -INFINITY, ok[3] ? ss[3] : -INFINITY)));
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p1 = __builtin_amdgcn_exp2f(fmaf(ss[r], a.k_sem, nm1));
                l1 += ok[r] ? p1 : 0.f;
                if (GEO) {
                    const float p2 = __builtin_amdgcn_exp2f(fmaf(sg[r], a.k_geo, nm2));
                    l2 += ok[r] ? p2 : 0.f;
                }
            }
        };
        if (n_here == BLK) tile_stats(std::false_type{});
        else tile_stats(std::true_type{});
        slot ^= 1;
    }
    // lanes j, j+16, j+32, j+48 hold disjoint row subsets of the same query
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
        l1 += __shfl_xor(l1, off);
        if (GEO) l2 += __shfl_xor(l2, off);
    }
    const float m1 = a.k_sem;
    float m2 = a.k_geo;
    if (!GEO) { m2 = NEG_BIG; l2 = 0.f; }   // "no rows": stays so under any merge
    if (q < a.B) {
        if (a.rowmax) a.rowmax[((int64_t)split * a.B + q) * 4 + g] = smax;   // before the lane merge
        if (g == 0) {
            f32x4 o = {m1, l1, m2, l2};
            *reinterpret_cast<f32x4*>(a.out + ((int64_t)split * a.B + q) * 4) = o;
        }
        if (TOPK) {
            const int64_t base = (((int64_t)split * a.B + q) * 4 + g) * MAX_TOPK;
#pragma unroll
            for (int k = 0; k < MAX_TOPK; ++k) {
                a.cand_val[base + k] = tk.v[TOPK ? k : 0];
                a.cand_idx[base + k] = tk.i[TOPK ? k : 0];
            }
        }
    }
}

// (n_parts,B,4) -> (B,4): exact log-sum-exp merge, fixed order.
__global__ void merge_stats_kernel(const float* parts, int n_parts, int64_t B, float* out) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= B) return;
    float m1 = NEG_BIG, l1 = 0.f, m2 = NEG_BIG, l2 = 0.f;
    for (int p = 0; p < n_parts; ++p) {
        const f32x4 s = *reinterpret_cast<const f32x4*>(parts + ((int64_t)p * B + q) * 4);
        merge_ml(m1, l1, s.x, s.y);
        merge_ml(m2, l2, s.z, s.w);
    }
    f32x4 o = {m1, l1, m2, l2};
    *reinterpret_cast<f32x4*>(out + q * 4) = o;
}

// The same merge with one WAVE per query, for the many-split launches of small batches (a
// thread walking 1000+ parts one dependent load at a time takes 0.4 ms): lane l folds parts
// l, l+64, ..., then a fixed butterfly of shuffles.
__global__ __launch_bounds__(256) void merge_stats_wave_kernel(const float* __restrict__ parts,
                                                               int n_parts, int64_t B,
                                                               float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= B) return;
    float m1 = NEG_BIG, l1 = 0.f, m2 = NEG_BIG, l2 = 0.f;
    for (int p = lane; p < n_parts; p += 64) {
        const f32x4 s = *reinterpret_cast<const f32x4*>(parts + ((int64_t)p * B + q) * 4);
        merge_ml(m1, l1, s.x, s.y);
        merge_ml(m2, l2, s.z, s.w);
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        merge_ml(m1, l1, __shfl_xor(m1, off), __shfl_xor(l1, off));
        merge_ml(m2, l2, __shfl_xor(m2, off), __shfl_xor(l2, off));
    }
    if (lane == 0) {
        f32x4 o = {m1, l1, m2, l2};
        *reinterpret_cast<f32x4*>(out + q * 4) = o;
    }
}

// top-k of n_cand candidates per query (values desc, ties -> lower index), k <= 16.
// One thread per query; candidate lists are tiny (n_parts * 64 or n_parts * k entries).
__global__ void merge_topk_kernel(const float* cval, const int32_t* cidx32, const int64_t* cidx64,
                                  int n_parts, int64_t B, int per_part, int k, int64_t row_offset,
                                  float* oval, int64_t* oidx) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= B) return;
    float bv[MAX_TOPK];
    int64_t bi[MAX_TOPK];
    for (int j = 0; j < MAX_TOPK; ++j) { bv[j] = -INFINITY; bi[j] = INT64_MAX; }
    for (int p = 0; p < n_parts; ++p) {
        const int64_t base = ((int64_t)p * B + q) * per_part;
        for (int c = 0; c < per_part; ++c) {
            const float v = cval[base + c];
            const int64_t i = cidx32 ? (cidx32[base + c] == 0x7fffffff
                                            ? INT64_MAX : (int64_t)cidx32[base + c] + row_offset)
                                     : cidx64[base + c];
            if (i == INT64_MAX) continue;
            // insert if better than the current worst
            if (v > bv[k - 1] || (v == bv[k - 1] && i < bi[k - 1])) {
                int j = k - 1;
                while (j > 0 && (v > bv[j - 1] || (v == bv[j - 1] && i < bi[j - 1]))) {
                    bv[j] = bv[j - 1]; bi[j] = bi[j - 1]; --j;
                }
                bv[j] = v; bi[j] = i;
            }
        }
    }
    for (int j = 0; j < k; ++j) { oval[q * k + j] = bv[j]; oidx[q * k + j] = bi[j] == INT64_MAX ? -1 : bi[j]; }
}

// pass 1: workgroups per CU (4 = what the 33 KB of LDS allow; fewer by padding the allocation:
// measured 3 and 2 per CU slower, tools/README.md)
constexpr int P1_WG_PER_CU = 4;
constexpr int SCAN_LDS_BYTES = (2 * BLK * KEY_DIM + 2 * 64) * 4;

}  // namespace range_hip
