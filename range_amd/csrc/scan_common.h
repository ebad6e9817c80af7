// Kernel B of the RANGE engine: streaming soft-attention over the embedding bank.
//
// Reference semantics (range/range.py:213-217, 231-238): for every query
//     H = softmax_N(tau_sem * e . K^T) @ V,   G = softmax_N(tau_geo * x . X^T) @ V,
//     M = (1-beta) * G + beta * H
// with N = ALL bank rows (dense soft attention, no top-k truncation).  The reference materialises
// two (B,N) probability matrices and multiplies each with V; here:
//
//   pass 1  scan_stats_kernel     per query running (max, sum-exp) of both logit rows; the raw
//                                 semantic logits are kept in HBM (4 B per (query,row) pair)
//   pass 2  attend_stored_kernel  reads them back, forms ONE combined weight
//                                 w = beta*p_sem + (1-beta)*p_geo and accumulates w @ V once
//                                 (2572 FLOP per pair over both passes instead of 4614)
//           attend_kernel         the same, recomputing the logits (when they were not kept)
//
// Both passes are FP32-MFMA bound (v_mfma_f32_16x16x4_f32: exact f32 products, bitwise an fmaf
// chain), not HBM bound - see DESIGN.md.  Work decomposition (identical in both passes):
//
//   workgroup = 4 waves = 64 queries; wave w owns queries 16w..16w+15 and, in pass 2, the FULL
//   1024-wide output row of each (64 accumulator tiles of 16x16 = 256 VGPRs).  Bank rows arrive
//   in blocks of 16 through LDS by LDS-DMA (global_load_lds, no VGPR staging) and are shared by
//   the 4 waves.  The logit tile is computed TRANSPOSED, S^T = K_blk . Q^T (bank row on the MFMA
//   row index, query on the lane), so its accumulator registers are directly the A operand of the
//   w @ V product - no LDS round trip and no inter-wave exchange for the weights.
//
//   grid = (query tiles) x (bank splits); a split is a contiguous range of 16-row blocks.  Because
//   pass 2 uses GLOBAL softmax statistics its per-split partial outputs simply add, so splits
//   give full-chip occupancy for any batch size and the same kernel serves a row-sharded bank.
//   blockIdx is mapped so that the workgroups resident on one XCD stream the SAME split(s)
//   (decode_block): the bank rows are fetched once per XCD L2, not once per CU.
// This header: what both passes (pass1.h, pass2.h) and the top-k scans share - launch arguments, the
// slab map of the partial outputs, the transposed logit tile and the LDS-DMA tile movers.
#pragma once
#include "engine_prims.h"
#include "host_plan.h"

namespace range_hip {

struct ScanArgs {
    const float* keys;     // (n_pad,256)
    const float* xyz4;     // (n_pad,4)
    const float* values;   // (n_pad,1024)   (pass 2)
    const float* ehat;     // (B,256)
    const float* xq;       // (B,4)
    const float* stats;    // (B,4) global stats (pass 2)
    float* out;            // pass 1: (nsplit,B,4) ; pass 2: (nsplit,B,1024)
    float* cand_val;       // pass 1 top-k candidates (nsplit,B,4,K) or null
    int32_t* cand_idx;
    int64_t B;
    int64_t n_valid;       // real bank rows
    int32_t n_blocks;      // ceil(n_valid/16)
    int32_t n_qtiles;
    int32_t n_splits;
    float k_sem;           // tau_sem * log2(e)
    float k_geo;           // tau_geo * log2(e)
    float beta;
    unsigned long long* diag;   // diagnostic build only: per (workgroup, wave) cycle sums
    // kept logits: the raw semantic dot products of pass 1, one 1 KB tile per (query tile, bank
    // block, wave) in accumulator-register order (lane-linear float4).  Pass 1 writes them when
    // non-null; attend_stored_kernel reads them instead of recomputing K . Q^T.
    float* logits;
    int32_t qt_offset;          // pass 2 on a sub-range of the scanned queries: first query / 64
    // pass 1, optional: (nsplit,B,4) largest semantic similarity each lane group met - disjoint
    // row subsets, so the 16th largest of a query's entries bounds its 16th best similarity from
    // below (the threshold of topk_from_logits_kernel)
    float* rowmax;
    // pass 2, stream-K decomposition (round 5): > 0 = the launch has exactly this many workgroups, each
    // walking a contiguous range of (query tile, bank block) units per bank column (SlabMap below);
    // 0 = one workgroup per (bank split, query tile) item (decode_block: the bf16-plane kernel, the
    // diagnostic launches)
    int32_t sk_groups;
    int32_t sk_cols;       // bank columns of the stream-K walk (>= 1)
};

// Where pass 2 leaves its partial outputs, and how their consumers find the parts of a query.
//   split-major (sk_groups == 0): n_parts planes of (B, 1024): part p of query q at (p B + q) 1024.
//   stream-K    (sk_groups  > 0): the bank's blocks are cut into sk_cols COLUMNS (contiguous, near-
//     equal: column c = blocks [c n_blocks / C, (c+1) n_blocks / C)), visited one after the other by
//     ALL workgroups - a column's rows (the values above all: 4 KB per row) are then re-read by the
//     workgroups while they are in the Infinity Cache; one column for a bank or shard that fits it.
//     Inside a column the units u = qtile * column_blocks + block, qtile-major, are cut into
//     sk_groups contiguous, near-equal ranges [start(w), start(w+1)), start(w) = floor(w U / G):
//     workgroup w walks its range in order - at most the tail of one query tile, whole tiles, the head
//     of another - and writes one (64, 1024) slab per query tile it touches, slab index
//     c (G + n_qtiles) + w + qtile (unique: every next segment of the walk increases w or qtile).
//     The parts of query tile qt in column c are the slabs w + qt for w = owner(qt cb) ..
//     owner((qt + 1) cb - 1), in block order; owner(u) = floor(((u + 1) G - 1) / U).  With G = the CUs
//     every workgroup has the same work (+- one block per column): no last partial round,
//     C (G + n_qtiles) slabs instead of n_splits n_qtiles, and a workgroup's fixed costs (~7.5 us:
//     first tiles, 256 KB of stores, dispatch) paid 1-2 times per CU and column.
struct SlabMap {
    int32_t n_parts;      // split-major: planes
    int32_t sk_groups;    // stream-K: workgroups of the launch (0 = split-major)
    int32_t n_blocks;
    int32_t n_qtiles;
    int32_t sk_cols;
};
using range_host::sk_owner;         // (host_plan.h: the partition arithmetic, also run under sanitizers on the CPU)
using range_host::sk_start, range_host::sk_col_begin;
// parts of query q in column c (split-major: the one "column" holds all planes): float4 index of the
// first, the stride between parts and their number
__device__ __forceinline__ void slab_parts(const SlabMap& m, int64_t B, int64_t q, int c, int64_t& first4, int64_t& stride4, int& count) {
    if (m.sk_groups == 0) {
        first4 = q * (VAL_DIM / 4);
        stride4 = B * (VAL_DIM / 4);
        count = m.n_parts;
        return;
    }
    const int64_t cb = sk_col_begin(c + 1, m.n_blocks, m.sk_cols) - sk_col_begin(c, m.n_blocks, m.sk_cols);
    const int64_t qt = q / QTILE, U = (int64_t)m.n_qtiles * cb;
    const int64_t w0 = sk_owner(qt * cb, U, m.sk_groups), w1 = sk_owner((qt + 1) * cb - 1, U, m.sk_groups);
    first4 = (((int64_t)c * (m.sk_groups + m.n_qtiles) + w0 + qt) * QTILE + (q - qt * QTILE)) * (VAL_DIM / 4);
    stride4 = (int64_t)QTILE * (VAL_DIM / 4);
    count = (int)(w1 - w0) + 1;
}
__device__ __forceinline__ int slab_cols(const SlabMap& m) { return m.sk_groups == 0 ? 1 : m.sk_cols; }

// float offset of the kept-logit tile of (query tile, bank block, wave)
__device__ __forceinline__ int64_t logit_tile(int64_t qtile, int32_t n_blocks, int block, int wave) {
    return ((qtile * n_blocks + block) * 4 + wave) * 256;
}

// blockIdx -> (split, query tile).  Work items are numbered split-major (item = split * n_qtiles +
// tile).  Blocks b and b+8 share an XCD (measured: XCC_ID == blockIdx % 8), so the blocks of XCD x
// (b = 8j + x) take a CONTIGUOUS run of items: the workgroups resident on one XCD then stream the
// same one or two splits and the bank rows are fetched once per XCD L2, not once per CU.
// Bijective for any item count: XCD x owns cnt(x) = q + (x < r) items, total = 8q + r.
// decode_item: the same for block number b of a persistent launch's walk b = blockIdx, blockIdx + grid, ...
// (a grid that is a multiple of 8 keeps b % 8, the XCD, along the walk).
__device__ __forceinline__ void decode_item(const ScanArgs& a, int b, int& split, int& qt) {
    const int total = a.n_splits * a.n_qtiles;
    const int x = b & 7, j = b >> 3;
    const int q = total >> 3, r = total & 7;
    const int item = x * q + (x < r ? x : r) + j;
    split = item / a.n_qtiles;
    qt = item - split * a.n_qtiles;
}
__device__ __forceinline__ void decode_block(const ScanArgs& a, int& split, int& qt) { decode_item(a, (int)blockIdx.x, split, qt); }

struct QFrag {
    f32x4 q[16];   // B operand of S^T = K . Q^T: lane (j = query, g) holds Q[j][16s + 4g + 0..3]
    float xq;      // geo head: xq[j][g]
};

__device__ __forceinline__ void load_qfrag(QFrag& f, const float* ehat, const float* xq, int64_t B,
                                           int64_t q, int g) {
    const int64_t qq = q < B ? q : B - 1;
    const f32x4* row = reinterpret_cast<const f32x4*>(ehat + qq * KEY_DIM);
#pragma unroll
    for (int s = 0; s < 16; ++s) f.q[s] = row[4 * s + g];
    f.xq = xq[qq * 4 + g];
}

// The query fragments come from ordinary global loads that hipcc counts; "using" them here puts
// its vmcnt wait for them in front of the main loop.  Otherwise the wait lands at their first use
// INSIDE the loop as vmcnt(0) and drains the hand-counted LDS-DMA ring every iteration.
__device__ __forceinline__ void pin_qfrag(QFrag& f) {
#pragma unroll
    for (int s = 0; s < 16; ++s) asm volatile("" : "+v"(f.q[s]));
    asm volatile("" : "+v"(f.xq));
}

// One 16-row block of transposed logits.  kt: LDS K tile [16][256] f32 whose 16-byte chunks were
// permuted at load time (chunk c of row R sits at position c ^ R, see issue_k_tile), which makes
// the ds_read_b128 below bank-conflict free.  The k index is consumed in a permuted order that is
// identical for both operands.  The 64 MFMAs of a tile form ONE dependent chain on a single
// accumulator: back-to-back MFMAs that accumulate into their own result issue at full rate on
// gfx950 (tools/micro/mfma_f32_chains.hip: 99 % with one chain), so the sum needs no VALU adds
// and every kernel that forms logits (both passes, the top-k scans) gets the same value.

// Accumulators of one transposed logit tile: the semantic chain and the geographic tile.
struct QKAcc {
    f32x4 a0, g;
    __device__ __forceinline__ float sem(int r) const { return a0[r]; }
    __device__ __forceinline__ void fence() {   // MFMA results -> VALU readers
        asm volatile("s_nop 15" : "+v"(a0), "+v"(g));
    }
};

// Per-lane LDS byte offsets of the K-tile reads (relative to the tile): with R = this lane's bank
// row and chunk index c = 4s + g, the swizzled position is c ^ R = 4(s ^ (R>>2)) + (g ^ (R&3));
// for s = 4a + b that is base[b] + 256*a bytes, so 4 VGPRs + immediates address all 16 reads.
struct KAddr {
    uint32_t b[4];
    uint32_t x;
    __device__ __forceinline__ void init(int lane) {
        const int g = lane >> 4;
        const int R = pi_row(lane & 15);
#pragma unroll
        for (int bb = 0; bb < 4; ++bb)
            b[bb] = (uint32_t)(R * (KEY_DIM * 4) + 64 * (bb ^ (R >> 2)) + 16 * (g ^ (R & 3)));
        x = (uint32_t)((R * 4 + g) * 4);
    }
};

struct KFirst { f32x4 k0, k1; float xa; };   // the reads of a tile's first two steps, issued early

template <bool GEO>
__device__ __forceinline__ KFirst qk_first_reads(const char* kt, const char* xt, const KAddr& ka_) {
    KFirst r;
    r.k0 = *reinterpret_cast<const f32x4*>(kt + ka_.b[0]);
    r.k1 = *reinterpret_cast<const f32x4*>(kt + ka_.b[1]);
    r.xa = GEO ? *reinterpret_cast<const float*>(xt + ka_.x) : 0.f;
    return r;
}

// hook(s) is inlined after the MFMAs of step s (used to start the next phase's LDS reads early).
template <bool GEO, class Hook>
__device__ __forceinline__ void qk_mfma(const char* kt, const KFirst& first, const KAddr& ka_,
                                        const QFrag& f, QKAcc& c, Hook&& hook) {
    // asm statements are scheduling boundaries for hipcc, so the LDS reads stay where the source
    // puts them: 16-byte K reads (4 k-steps each) two steps ahead of the MFMAs that hide their latency.
    f32x4 kn = first.k0, kn2 = first.k1;
    const float xa = first.xa;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const f32x4 ka = kn;
        kn = kn2;
        if (s < 14) kn2 = *reinterpret_cast<const f32x4*>(kt + ka_.b[(s + 2) & 3] + 256 * ((s + 2) >> 2));
        if (s == 0) mfma_v_first(c.a0, ka.x, f.q[s].x);
        else mfma_v(c.a0, ka.x, f.q[s].x);
        mfma_v(c.a0, ka.y, f.q[s].y);
        mfma_v(c.a0, ka.z, f.q[s].z);
        mfma_v(c.a0, ka.w, f.q[s].w);
        hook(s);
    }
    if (GEO) mfma_v_first(c.g, xa, f.xq);
    else c.g = f32x4{0.f, 0.f, 0.f, 0.f};
}

// One K tile (16 rows x 1 KB) + its X tile (16 x 4 f32).  Wave w moves rows 4w..4w+3, one
// dwordx4 DMA per row: lane ln fetches chunk (ln ^ R) of row R and lands at LDS position ln (the
// LDS side of LDS-DMA is always lane-linear; the swizzle lives on the source address).
// Every wave also issues the (identical) 256-byte X copy so that all waves keep the same count
// of outstanding vector-memory operations: 5 per tile.
// kt_lds / xt_lds are LDS byte addresses; swz = (lane ^ 4*wave) precomputed.
__device__ __forceinline__ void issue_k_tile(const float* keys, const float* xyz4, int64_t row0,
                                             uint32_t kt_lds, uint32_t xt_lds, int wave, int lane,
                                             int swz) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int R = 4 * wave + rr;
        dma_b128(keys + (row0 + R) * KEY_DIM, (uint32_t)((swz ^ rr) << 4), kt_lds + R * (KEY_DIM * 4));
    }
    dma_b32(xyz4 + row0 * 4, (uint32_t)(lane << 2), xt_lds);
}

// One 8-row half block of V (32 KB, row-major, linear): 32 pieces of 1 KB, 8 per wave.
__device__ __forceinline__ void issue_v_half(const float* values, int64_t row0, uint32_t vslot_lds,
                                             int wave, int lane) {
#pragma unroll
    for (int ii = 0; ii < 8; ++ii) {
        const int i = 8 * wave + ii;
        dma_b128(values + (row0 + (i >> 2)) * VAL_DIM + (i & 3) * 256, (uint32_t)(lane << 4),
                 vslot_lds + i * 1024);
    }
}

}  // namespace range_hip
