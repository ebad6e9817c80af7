// Pass 1's softmax statistics at OTHER temperatures, from the logits a scan kept (scan_common.h:
// ScanArgs::logits): the raw semantic dot products are un-scaled, so the statistics of any (tau_sem,
// tau_geo) follow from one read of them - no e . K^T, no key stream, no LDS ring.  HBM-bound: 4 B per
// (query, row) pair whatever the number of temperature pairs a launch serves (up to KEPT_MAX_PAIRS).
//
// Every pair's parts are, bit for bit, what scan_stats_kernel<GEO, false> (pass1.h; both temperatures
// <= 43: the constant shift) or sharp_scan_stats_kernel<GEO> (pass1_sharp.h; either above: the running
// maximum for both heads) writes for the same queries and split count: the same decomposition - one
// workgroup of 4 waves per (bank split, query tile), wave w and lane (j, g) own the elements they own
// there -, the same fmaf / exp2 sequences tile by tile with r = 0..3 inside a tile, the same lane merge.
// The geographic logit of a tile is the one v_mfma_f32_16x16x4_f32 of QKAcc::g, its A operand read
// straight from xyz4 in global memory (one float per lane, 256 B per tile).
#pragma once
#include <type_traits>

#include "pass1.h"

namespace range_hip {

constexpr int KEPT_MAX_PAIRS = 8;     // temperature pairs of one launch
constexpr int KEPT_TILES_IN_FLIGHT = 8;   // 1 KB tile loads a wave keeps in flight (as topk_from_logits_kernel)

struct KeptStatsArgs {
    const float* logits;   // the kept tiles (scan_common.h: logit_tile)
    const float* xyz4;     // (n_pad,4)
    const float* xq;       // (B,4)
    float* out;            // (pair, split, B, 4)
    int64_t B;
    int64_t n_valid;       // real bank rows
    int32_t n_blocks;      // ceil(n_valid/16)
    int32_t n_qtiles;
    int32_t n_splits;
    int32_t qt_offset;     // first query / 64 in the kept scan
    uint32_t sharp_mask;   // bit p: pair p takes the running-max form (host_plan.h: kept_pair_shift)
    uint32_t geo_mask;     // bit p: pair p has a geographic head
    float k_sem[KEPT_MAX_PAIRS];   // tau_sem * log2(e)
    float k_geo[KEPT_MAX_PAIRS];   // tau_geo * log2(e)
};

// merge_ml (engine_prims.h) for the lane merge, written out as sharp_scan_stats_kernel's generated code
// evaluates it: `l * a + l2 * b` is contracted there to fma(l, a, round(l2 * b)); which product hipcc
// folds into the fma depends on the code around the expression (here it chose neither in one of the two
// steps), so the product and the fma are spelled out.  tests/test_gpu_temperature_sweep.py compares the
// bits with that kernel's.
__device__ __forceinline__ void merge_ml_lanes(float& m, float& l, float m2, float l2) {
    const float mm = fmaxf(m, m2);
    // (plain C++: hipcc then keeps the wait state a v_exp_f32 result needs before its next use, which an
    // asm statement would not get; a product that feeds fmaf's addend cannot be contracted further)
    const float t2 = l2 * __builtin_amdgcn_exp2f(m2 - mm);
    l = fmaf(l, __builtin_amdgcn_exp2f(m - mm), t2);
    m = mm;
}

// (m, l) of both heads for one pair; the constant form only uses l1 / l2
struct KeptPairStats { float m1, l1, m2, l2; };

// NP: pairs of the launch; GEO: some pair has a geographic head (the tile's geographic logit is formed)
template <int NP, bool GEO>
__global__ __launch_bounds__(256) void kept_stats_kernel(KeptStatsArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4;
    const int split = blockIdx.x / a.n_qtiles;
    const int qt = blockIdx.x - split * a.n_qtiles;
    const int b0 = part_begin(split, a.n_blocks, a.n_splits);
    const int b1 = part_begin(split + 1, a.n_blocks, a.n_splits);
    const int64_t q = (int64_t)qt * QTILE + wave * 16 + (lane & 15);

    // what pass 1 stored from c.sem(0..3): lane-linear float4 of tile (query tile, block, wave)
    const float* base = a.logits + logit_tile((int64_t)qt + a.qt_offset, a.n_blocks, 0, wave) + 4 * lane;
    // A operand of the geographic tile: xyz4[block * 16 + pi_row(lane & 15)][g] (scan_common.h: KAddr::x)
    const float* xbase = a.xyz4 + pi_row(lane & 15) * 4 + g;
    float fxq = 0.f;
    if (GEO) {
        fxq = a.xq[(q < a.B ? q : a.B - 1) * 4 + g];
        asm volatile("" : "+v"(fxq));
    }

    KeptPairStats st[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) st[p] = KeptPairStats{NEG_BIG, 0.f, NEG_BIG, 0.f};

    // statistics of one tile for every pair.  Only the bank's last block can hold pad rows: every other
    // tile takes the unmasked form
    auto tile_stats = [&](const f32x4 ss, const f32x4 sg, const int n_here, auto masked_tag) __attribute__((always_inline)) {
        constexpr bool MASKED = decltype(masked_tag)::value;
        bool ok[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) ok[r] = !MASKED || pi_row(4 * g + r) < n_here;
        // (the running-max form; fmaxf drops a NaN logit from the maximum, the exp2 term keeps it in l)
        const float smx = fmaxf(fmaxf(ok[0] ? ss[0] : -INFINITY, ok[1] ? ss[1] : -INFINITY),
                                fmaxf(ok[2] ? ss[2] : -INFINITY, ok[3] ? ss[3] : -INFINITY));
        const float gmx = fmaxf(fmaxf(ok[0] ? sg[0] : -INFINITY, ok[1] ? sg[1] : -INFINITY),
                                fmaxf(ok[2] ? sg[2] : -INFINITY, ok[3] ? sg[3] : -INFINITY));
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const float k_sem = a.k_sem[p], k_geo = a.k_geo[p];
            const bool geo = GEO && ((a.geo_mask >> p) & 1u);
            KeptPairStats& s = st[p];
            if ((a.sharp_mask >> p) & 1u) {
                // sharp_scan_stats_kernel: one rescale per tile
                const float mn1 = fmaxf(s.m1, k_sem * smx);
                float sum1 = 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p1 = __builtin_amdgcn_exp2f(fmaf(ss[r], k_sem, -mn1));
                    sum1 += ok[r] ? p1 : 0.f;
                }
                s.l1 = fmaf(s.l1, __builtin_amdgcn_exp2f(s.m1 - mn1), sum1);
                s.m1 = mn1;
                if (geo) {
                    const float mn2 = fmaxf(s.m2, k_geo * gmx);
                    float sum2 = 0.f;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float p2 = __builtin_amdgcn_exp2f(fmaf(sg[r], k_geo, -mn2));
                        sum2 += ok[r] ? p2 : 0.f;
                    }
                    s.l2 = fmaf(s.l2, __builtin_amdgcn_exp2f(s.m2 - mn2), sum2);
                    s.m2 = mn2;
                }
            } else {
                // scan_stats_kernel: the constant shift m = k
                const float nm1 = -k_sem, nm2 = -k_geo;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p1 = __builtin_amdgcn_exp2f(fmaf(ss[r], k_sem, nm1));
                    s.l1 += ok[r] ? p1 : 0.f;
                    if (geo) {
                        const float p2 = __builtin_amdgcn_exp2f(fmaf(sg[r], k_geo, nm2));
                        s.l2 += ok[r] ? p2 : 0.f;
                    }
                }
            }
        }
    };

    // the geographic logit of a tile: the bits of QKAcc::g (scan_common.h: qk_mfma)
    auto geo_tile = [&](const float xa) __attribute__((always_inline)) {
        f32x4 sg = {0.f, 0.f, 0.f, 0.f};
        if (GEO) {
            mfma_v_first(sg, xa, fxq);
            asm volatile("s_nop 15" : "+v"(sg));      // MFMA result -> VALU readers (QKAcc::fence)
        }
        return sg;
    };

    // pad rows exist in the bank's last block only: it is taken alone, behind the unmasked stream
    const int n_last = (int)(a.n_valid - (int64_t)(a.n_blocks - 1) * BLK);      // valid rows of the bank's last block
    const int b1u = (b1 == a.n_blocks && n_last < BLK) ? b1 - 1 : b1;
    constexpr int U = KEPT_TILES_IN_FLIGHT;
    for (int b = b0; b < b1u; b += U) {
        f32x4 v[U];
        float xa[U];
        // (the small location reads first: the tiles are then waited for one by one, in order)
#pragma unroll
        for (int u = 0; u < U; ++u) xa[u] = GEO ? xbase[(int64_t)(b + u < b1u ? b + u : b1u - 1) * (BLK * 4)] : 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u)
            v[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(base + (int64_t)(b + u < b1u ? b + u : b1u - 1) * 1024));
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (b + u < b1u) tile_stats(v[u], geo_tile(xa[u]), BLK, std::false_type{});
    }
    if (b1u < b1) {
        const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(base + (int64_t)b1u * 1024));
        const float xa = GEO ? xbase[(int64_t)b1u * (BLK * 4)] : 0.f;
        tile_stats(v, geo_tile(xa), n_last, std::true_type{});
    }

    // lanes j, j+16, j+32, j+48 hold disjoint row subsets of the same query
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const bool geo = GEO && ((a.geo_mask >> p) & 1u);
        float m1, l1 = st[p].l1, m2, l2 = st[p].l2;
        if ((a.sharp_mask >> p) & 1u) {
            m1 = st[p].m1;
            m2 = st[p].m2;
#pragma unroll
            for (int off = 16; off <= 32; off <<= 1) {
                merge_ml_lanes(m1, l1, __shfl_xor(m1, off), __shfl_xor(l1, off));
                if (geo) merge_ml_lanes(m2, l2, __shfl_xor(m2, off), __shfl_xor(l2, off));
            }
        } else {
#pragma unroll
            for (int off = 16; off <= 32; off <<= 1) {
                l1 += __shfl_xor(l1, off);
                if (geo) l2 += __shfl_xor(l2, off);
            }
            m1 = a.k_sem[p];
            m2 = a.k_geo[p];
        }
        if (!geo) { m2 = NEG_BIG; l2 = 0.f; }   // "no rows": stays so under any merge
        if (q < a.B && g == 0) {
            f32x4 o = {m1, l1, m2, l2};
            *reinterpret_cast<f32x4*>(a.out + (((int64_t)p * a.n_splits + split) * a.B + q) * 4) = o;
        }
    }
}

}  // namespace range_hip
