// Pass 1 for SHARP temperatures (above RANGE_MAX_TAU): the softmax statistics with a RUNNING maximum.
// The constant shift m = tau * log2(e) of scan_stats_kernel (pass1.h) needs 2^(-2m) to stay a normal
// float32; beyond tau = 43 a sharp softmax underflows as a whole (a query whose best similarity is 0.2
// has its largest term at 2^(-0.8 m)).  Here every lane keeps (m, l) with m the largest scaled logit
// it has met.  Pass 2 and every merge of statistics take their shift per query from the statistics
// (pass2.h: load_weight_consts; merge_ml), so nothing but this kernel changes with the shift.
#pragma once
#include <type_traits>

#include "pass1.h"

namespace range_hip {

// Decomposition, LDS ring, logit tile, kept-logit store, a.rowmax and the pad-row masking are those of
// scan_stats_kernel<GEO, false>; there are no in-scan top-k lists here.
template <bool GEO>
__global__ __launch_bounds__(256) void sharp_scan_stats_kernel(ScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // LDS: K ring 2 x [16][256] f32 | X ring 2 x [16][4] f32 (SCAN_LDS_BYTES: four workgroups per CU)
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

    // (m, l) per lane and head, in the units pass 2 expects: m is the largest k * s met so far,
    // l = sum 2^(k s - m).  One rescale per TILE of 4 rows, not per element.  "No rows" is
    // (NEG_BIG, 0), which merge_ml absorbs.
    float m1 = NEG_BIG, l1 = 0.f, m2 = NEG_BIG, l2 = 0.f;
    float smax = -INFINITY;      // largest similarity of this lane's rows (a.rowmax)

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
            __builtin_nontemporal_store(ss, reinterpret_cast<f32x4*>(a.logits + logit_tile((int64_t)qt + a.qt_offset, a.n_blocks, b0 + t, wave) + 4 * lane));
        // statistics of this tile.  Only the bank's last block can hold pad rows: every other
        // tile takes the unmasked form
        const int64_t row0 = (int64_t)(b0 + t) * BLK;
        const int n_here = (int)(a.n_valid - row0 < BLK ? a.n_valid - row0 : BLK);   // valid rows
        auto tile_stats = [&](auto masked_tag) __attribute__((always_inline)) {
            constexpr bool MASKED = decltype(masked_tag)::value;
            bool ok[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) ok[r] = !MASKED || pi_row(4 * g + r) < n_here;
            // fmaxf drops a NaN logit from the maximum; the exp2(fma(NaN ...)) term below keeps it in l
            const float smx = fmaxf(fmaxf(ok[0] ? ss[0] : -INFINITY, ok[1] ? ss[1] : -INFINITY),
                                    fmaxf(ok[2] ? ss[2] : -INFINITY, ok[3] ? ss[3] : -INFINITY));
            if (a.rowmax) smax = fmaxf(smax, smx);
            const float mn1 = fmaxf(m1, a.k_sem * smx);
            float sum1 = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p1 = __builtin_amdgcn_exp2f(fmaf(ss[r], a.k_sem, -mn1));
                sum1 += ok[r] ? p1 : 0.f;
            }
            l1 = fmaf(l1, __builtin_amdgcn_exp2f(m1 - mn1), sum1);
            m1 = mn1;
            if (GEO) {
                const float gmx = fmaxf(fmaxf(ok[0] ? sg[0] : -INFINITY, ok[1] ? sg[1] : -INFINITY),
                                        fmaxf(ok[2] ? sg[2] : -INFINITY, ok[3] ? sg[3] : -INFINITY));
                const float mn2 = fmaxf(m2, a.k_geo * gmx);
                float sum2 = 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p2 = __builtin_amdgcn_exp2f(fmaf(sg[r], a.k_geo, -mn2));
                    sum2 += ok[r] ? p2 : 0.f;
                }
                l2 = fmaf(l2, __builtin_amdgcn_exp2f(m2 - mn2), sum2);
                m2 = mn2;
            }
        };
        if (n_here == BLK) tile_stats(std::false_type{});
        else tile_stats(std::true_type{});
        slot ^= 1;
    }
    const float smax_lane = smax;
    // lanes j, j+16, j+32, j+48 hold disjoint row subsets of the same query: different m, exact merge
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
        merge_ml(m1, l1, __shfl_xor(m1, off), __shfl_xor(l1, off));
        if (GEO) merge_ml(m2, l2, __shfl_xor(m2, off), __shfl_xor(l2, off));
    }
    if (!GEO) { m2 = NEG_BIG; l2 = 0.f; }   // "no rows": stays so under any merge
    if (q < a.B) {
        if (a.rowmax) a.rowmax[((int64_t)split * a.B + q) * 4 + g] = smax_lane;   // before the lane merge
        if (g == 0) {
            f32x4 o = {m1, l1, m2, l2};
            *reinterpret_cast<f32x4*>(a.out + ((int64_t)split * a.B + q) * 4) = o;
        }
    }
}

}  // namespace range_hip
