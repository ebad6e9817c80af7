// Pass 1 for the CUs that pass 2 occupies (forward_host.h: the chunked forward): the statistics and the kept
// logits of scan_stats_kernel<GEO, false>, bit for bit, from a workgroup small enough to sit NEXT TO one
// of attend_stored_kernel - that kernel takes 344 of a SIMD's 512 registers per lane and 139 776 of the
// CU's 163 840 bytes of LDS, and has one wave per SIMD whose MFMA stream leaves the matrix pipe idle
// 9 % of the time.  What differs from scan_stats_kernel:
//   - the key ring holds HALF tiles, [16 rows][128 floats] a slot (16 896 B of LDS with the X ring instead of
//     33 280 B): steps 0-7 of the tile's MFMA chain read the first half-tile, steps 8-15 the second.  The
//     chunk swizzle c ^ R of issue_k_tile only touches the low four bits of the chunk index, so a half row is
//     closed under it and a lane's reads keep their bank-conflict-free positions;
//   - the launch is persistent: min(CUs, items) workgroups, each walking the (bank split, query tile) items
//     b, b + grid, ... in decode_item's numbering - one workgroup per CU, whatever else runs there.
// The 64 MFMAs of a tile stay ONE dependent chain on one accumulator in scan_stats_kernel's order (qk_mfma),
// the statistics of a tile are its expressions: that is what keeps the bits.
#pragma once
#include <type_traits>

#include "pass1.h"
#include "pass2.h"

namespace range_hip {

constexpr uint32_t BESIDE_HALF_BYTES = BLK * (KEY_DIM / 2) * 4;        // a half tile: 16 rows x 512 B
constexpr int BESIDE_LDS_BYTES = 2 * BESIDE_HALF_BYTES + 2 * 64 * 4;   // K ring of two half tiles | X ring 2 x [16][4] f32
static_assert(ATTEND_STORED_LDS_BYTES + BESIDE_LDS_BYTES <= 160 * 1024, "pass 1 must fit beside pass 2 in a CU's LDS");

// Per-lane LDS byte offsets of the half-tile reads (KAddr for rows of 512 B): step s = 8h + 4a + b of the
// chain reads b[b] + 256 a of half tile h.
struct KAddrHalf {
    uint32_t b[4];
    uint32_t x;
    __device__ __forceinline__ void init(int lane) {
        const int g = lane >> 4;
        const int R = pi_row(lane & 15);
#pragma unroll
        for (int bb = 0; bb < 4; ++bb)
            b[bb] = (uint32_t)(R * (KEY_DIM * 2) + 64 * (bb ^ (R >> 2)) + 16 * (g ^ (R & 3)));
        x = (uint32_t)((R * 4 + g) * 4);
    }
};

// Half h of one K tile: 16 half rows of 512 B.  A dwordx4 DMA of a wave moves 1 KB = two rows of the slot:
// wave w rows 4w .. 4w+3 in two of them; lane ln of DMA d fetches chunk ((ln & 31) ^ R) + 32 h of row
// R = 4w + 2d + (ln >> 5) and lands at position ln & 31 of that row.  voff[d]: the lane's source byte
// offset from row 4w + 2d of the tile, for half 0.
__device__ __forceinline__ void issue_k_half(const float* keys, int64_t row0, int half, uint32_t slot_lds, int wave,
                                             const uint32_t (&voff)[2]) {
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const int R0 = 4 * wave + 2 * d;
        dma_b128(keys + (row0 + R0) * KEY_DIM, voff[d] + (uint32_t)half * (KEY_DIM * 2), slot_lds + R0 * (KEY_DIM * 2));
    }
}

// Steps 8 H .. 8 H + 7 of qk_mfma's chain from half tile H (kh): the same reads two steps ahead, the same
// MFMAs in the same order on the accumulator a0.
template <int H>
__device__ __forceinline__ void qk_mfma_half(const char* kh, const KAddrHalf& ka_, const QFrag& f, f32x4& a0) {
    f32x4 kn = *reinterpret_cast<const f32x4*>(kh + ka_.b[0]);
    f32x4 kn2 = *reinterpret_cast<const f32x4*>(kh + ka_.b[1]);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const f32x4 ka = kn;
        kn = kn2;
        if (s < 6) kn2 = *reinterpret_cast<const f32x4*>(kh + ka_.b[(s + 2) & 3] + 256 * ((s + 2) >> 2));
        const int S = 8 * H + s;
        if (S == 0) mfma_v_first(a0, ka.x, f.q[S].x);
        else mfma_v(a0, ka.x, f.q[S].x);
        mfma_v(a0, ka.y, f.q[S].y);
        mfma_v(a0, ka.z, f.q[S].z);
        mfma_v(a0, ka.w, f.q[S].w);
    }
}

// at most 168 registers a lane (three waves' share of a SIMD's 512): what pass 2 leaves
template <bool GEO>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void scan_stats_beside_kernel(ScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint32_t lds0 = (uint32_t)(uintptr_t)RANGE_LPTR(smem);
    const uint32_t xring_lds = lds0 + 2 * BESIDE_HALF_BYTES;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4;
    KAddrHalf kaddr;
    kaddr.init(lane);
    uint32_t voff[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const int R = 4 * wave + 2 * d + (lane >> 5);
        voff[d] = (uint32_t)((lane >> 5) * (KEY_DIM * 4) + (((lane & 31) ^ R) << 4));
    }
    const float nm1 = -a.k_sem, nm2 = -a.k_geo;
    const int total = a.n_splits * a.n_qtiles;

    for (int vb = blockIdx.x; vb < total; vb += gridDim.x) {
        int split, qt;
        decode_item(a, vb, split, qt);
        const int b0 = part_begin(split, a.n_blocks, a.n_splits);
        const int nb = part_begin(split + 1, a.n_blocks, a.n_splits) - b0;
        const int64_t q = (int64_t)qt * QTILE + wave * 16 + (lane & 15);

        QFrag f;
        load_qfrag(f, a.ehat, a.xq, a.B, q, g);
        pin_qfrag(f);
        float l1 = 0.f, l2 = 0.f;     // (the constant shift: see scan_stats_kernel)

        // Phase p = 2t + h is half h of tile t and lives in ring slot h.  Phase p + 1 is requested right after
        // barrier p (every wave is then done with phase p - 1, whose slot it re-uses) and waited for before
        // barrier p + 1; the X tile of tile t travels with its first half into X slot t & 1 and is read in that
        // phase, so the next item's first request - issued by a wave that has passed this item's last barrier -
        // finds every reader of both slots it writes done.
        if (nb > 0) {
            issue_k_half(a.keys, (int64_t)b0 * BLK, 0, lds0, wave, voff);
            dma_b32(a.xyz4 + (int64_t)b0 * BLK * 4, (uint32_t)(lane << 2), xring_lds);
        }
        for (int t = 0; t < nb; ++t) {
            const int64_t row0 = (int64_t)(b0 + t) * BLK;
            QKAcc c;
            RANGE_WAIT_BARRIER(0);
            issue_k_half(a.keys, row0, 1, lds0 + BESIDE_HALF_BYTES, wave, voff);
            const float xa = GEO ? *reinterpret_cast<const float*>(smem + 2 * BESIDE_HALF_BYTES + (t & 1) * 256 + kaddr.x) : 0.f;
            qk_mfma_half<0>(smem, kaddr, f, c.a0);
            RANGE_WAIT_BARRIER(0);
            if (t + 1 < nb) {
                issue_k_half(a.keys, row0 + BLK, 0, lds0, wave, voff);
                dma_b32(a.xyz4 + (row0 + BLK) * 4, (uint32_t)(lane << 2), xring_lds + ((t + 1) & 1) * 256);
            }
            qk_mfma_half<1>(smem + BESIDE_HALF_BYTES, kaddr, f, c.a0);
            if (GEO) mfma_v_first(c.g, xa, f.xq);
            else c.g = f32x4{0.f, 0.f, 0.f, 0.f};
            c.fence();
            const f32x4 ss = {c.sem(0), c.sem(1), c.sem(2), c.sem(3)};
            const f32x4 sg = c.g;
            if (a.logits)   // (the next barrier's vmcnt(0) also covers this store)
                __builtin_nontemporal_store(ss, reinterpret_cast<f32x4*>(a.logits + logit_tile((int64_t)qt + a.qt_offset, a.n_blocks, b0 + t, wave) + 4 * lane));
            // statistics of this tile: scan_stats_kernel's, without its top-k lists and row maxima
            const int n_here = (int)(a.n_valid - row0 < BLK ? a.n_valid - row0 : BLK);   // valid rows
            auto tile_stats = [&](auto masked_tag) __attribute__((always_inline)) {
                constexpr bool MASKED = decltype(masked_tag)::value;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool ok = !MASKED || pi_row(4 * g + r) < n_here;
                    const float p1 = __builtin_amdgcn_exp2f(fmaf(ss[r], a.k_sem, nm1));
                    l1 += ok ? p1 : 0.f;
                    if (GEO) {
                        const float p2 = __builtin_amdgcn_exp2f(fmaf(sg[r], a.k_geo, nm2));
                        l2 += ok ? p2 : 0.f;
                    }
                }
            };
            if (n_here == BLK) tile_stats(std::false_type{});
            else tile_stats(std::true_type{});
        }
        // lanes j, j+16, j+32, j+48 hold disjoint row subsets of the same query
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
            l1 += __shfl_xor(l1, off);
            if (GEO) l2 += __shfl_xor(l2, off);
        }
        float m2 = a.k_geo;
        if (!GEO) { m2 = NEG_BIG; l2 = 0.f; }   // "no rows": stays so under any merge
        if (q < a.B && g == 0) {
            f32x4 o = {a.k_sem, l1, m2, l2};
            *reinterpret_cast<f32x4*>(a.out + ((int64_t)split * a.B + q) * 4) = o;
        }
    }
}

}  // namespace range_hip
