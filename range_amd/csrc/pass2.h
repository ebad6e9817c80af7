// Pass 2 of the two-pass soft attention (overview: scan_common.h): w @ V on recomputed or kept
// logits, and the reductions of its partial outputs.
#pragma once
#include "scan_common.h"

namespace range_hip {

// Diagnostic build only (attend_kernel<GEO, true>, never on the product path): s_memtime stamps
// around the two parts of a wait so that their cycles can be summed per wave.
__device__ __forceinline__ unsigned long long stamp() {
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    return t;
}
#define RANGE_WAIT_BARRIER_DIAG(n, vm, bar)                                   \
    do {                                                                      \
        const unsigned long long t0_ = stamp();                               \
        asm volatile("s_waitcnt vmcnt(" #n ") lgkmcnt(0)" ::: "memory");      \
        const unsigned long long t1_ = stamp();                               \
        asm volatile("s_barrier" ::: "memory");                               \
        const unsigned long long t2_ = stamp();                               \
        vm += t1_ - t0_; bar += t2_ - t1_;                                    \
    } while (0)
#define RANGE_WB(n, vm, bar)                                                  \
    do { if (DIAG) RANGE_WAIT_BARRIER_DIAG(n, vm, bar); else RANGE_WAIT_BARRIER(n); } while (0)

// 8 bank rows x 1024 columns of w @ V for this wave's 16 queries, as 16 steps of 8 MFMAs (4
// accumulator tiles x 2 rows).  Two devices keep the MFMA pipe fed with one wave per SIMD:
//  * hook(h), h = 0..59, is inlined after every second MFMA: scalar/vector work placed there in
//    pieces of <= ~6 instructions (one LDS-DMA for a later tile, a slice of the next block's
//    softmax weights) issues in the shadow of the 32-cycle MFMAs (an MFMA occupies the issue port
//    for 8 of its 32 cycles);
//  * the LAST two steps of a phase are not executed but handed on as a PvCarry (their V operands are
//    already in registers): the next phase runs them right after its barrier, behind the first LDS
//    reads of the new phase, so no LDS latency is exposed at a phase boundary.
struct PvCarry {          // the last PV_CARRY = 2 steps of a half (16 MFMAs = 512 cycles of cover)
    f32x4 v0a, v1a, v0b, v1b;
    float w0, w1;
    __device__ __forceinline__ void zero() {
        v0a = v1a = v0b = v1b = f32x4{0.f, 0.f, 0.f, 0.f};
        w0 = w1 = 0.f;
    }
};

struct PvOps { f32x4 v0, v1; };   // V operands of one step: rows 2g and 2g+1, 4 columns each

// operands of steps 0 and 1 of a half (the read pipeline is two steps deep)
__device__ __forceinline__ void pv_first_reads(const float* vslot, int lane, PvOps& s0, PvOps& s1) {
    const float* base = vslot + (2 * (lane >> 4)) * VAL_DIM + 4 * (lane & 15);
    s0.v0 = *reinterpret_cast<const f32x4*>(base);
    s0.v1 = *reinterpret_cast<const f32x4*>(base + VAL_DIM);
    s1.v0 = *reinterpret_cast<const f32x4*>(base + 64);
    s1.v1 = *reinterpret_cast<const f32x4*>(base + VAL_DIM + 64);
}

__device__ __forceinline__ void pv_exec_carry(f32x4 (&acc)[64], const PvCarry& c) {
    mfma_a(acc[56], c.w0, c.v0a.x);
    mfma_a(acc[57], c.w0, c.v0a.y);
    mfma_a(acc[58], c.w0, c.v0a.z);
    mfma_a(acc[59], c.w0, c.v0a.w);
    mfma_a(acc[56], c.w1, c.v1a.x);
    mfma_a(acc[57], c.w1, c.v1a.y);
    mfma_a(acc[58], c.w1, c.v1a.z);
    mfma_a(acc[59], c.w1, c.v1a.w);
    mfma_a(acc[60], c.w0, c.v0b.x);
    mfma_a(acc[61], c.w0, c.v0b.y);
    mfma_a(acc[62], c.w0, c.v0b.z);
    mfma_a(acc[63], c.w0, c.v0b.w);
    mfma_a(acc[60], c.w1, c.v1b.x);
    mfma_a(acc[61], c.w1, c.v1b.y);
    mfma_a(acc[62], c.w1, c.v1b.z);
    mfma_a(acc[63], c.w1, c.v1b.w);
}

// One step = 8 MFMAs: 4 accumulator tiles x 2 bank rows.  A phase has N steps: N = 16 is an 8-row half
// (attend_kernel: hook(h), h = 0..111), N = 32 a whole 16-row block in ONE phase (pass 2 on kept
// logits, whose V ring holds whole blocks: h = 0..239, h < 128 the first half) - one hand-over per
// block instead of two, the read pipeline runs through the half boundary, and every accumulator tile
// sees the same products in the same order as from two halves.  Step S goes over rows 0-7 (S < 16) or
// 8-15 of the rows at `base` with the weights w[W0 + 2 (S >> 4)], w[.. + 1].  v0/v1 = operands of step
// S, n0/n1 of step S+1; the last two steps are not executed but left there for the PvCarry.
// hook(8 S + i) runs after MFMA i of the step.  The sched_barriers pin each piece into its own MFMA
// gap: without them hipcc sinks the pieces behind groups of four MFMAs, where only the last MFMA's
// shadow (24 issue cycles) is left to hide them.
// (Template recursion, not a loop: 30 steps of 8 hooks are beyond what `#pragma unroll` unrolls in
// full before the hooks are folded, and a partly unrolled loop evaluates the hooks at run time.  The
// 14 steps of a half would unroll; they take the same path so that the step exists once.)
#define RANGE_PV_MFMA(tile, w, v, h)                 \
    mfma_a(acc[tile], w, v);                         \
    __builtin_amdgcn_sched_barrier(0);               \
    hook(h);                                         \
    __builtin_amdgcn_sched_barrier(0)
template <int S, int N, int W0, class Hook>
__device__ __forceinline__ void pv_step(const float* base, const f32x4& w, f32x4& v0, f32x4& v1,
                                        f32x4& n0, f32x4& n1, f32x4 (&acc)[64], Hook& hook) {
    if constexpr (S < N - 2) {
        // lane (j,g) reads V[row 2g+rr][64T + 4j .. +3]: one ds_read_b128 feeds 4 accumulator
        // tiles; the reads of step S+2 sit in front of step S's 8 MFMAs (512 cycles of cover)
        constexpr int T = S & 15, S2 = S + 2;
        const float* src = base + (S2 >> 4) * 8 * VAL_DIM + 64 * (S2 & 15);
        const f32x4 m0 = *reinterpret_cast<const f32x4*>(src);
        const f32x4 m1 = *reinterpret_cast<const f32x4*>(src + VAL_DIM);
        const float w0 = w[W0 + 2 * (S >> 4)], w1 = w[W0 + 2 * (S >> 4) + 1];
        RANGE_PV_MFMA(4 * T + 0, w0, v0.x, 8 * S + 0);
        RANGE_PV_MFMA(4 * T + 1, w0, v0.y, 8 * S + 1);
        RANGE_PV_MFMA(4 * T + 2, w0, v0.z, 8 * S + 2);
        RANGE_PV_MFMA(4 * T + 3, w0, v0.w, 8 * S + 3);
        RANGE_PV_MFMA(4 * T + 0, w1, v1.x, 8 * S + 4);
        RANGE_PV_MFMA(4 * T + 1, w1, v1.y, 8 * S + 5);
        RANGE_PV_MFMA(4 * T + 2, w1, v1.z, 8 * S + 6);
        RANGE_PV_MFMA(4 * T + 3, w1, v1.w, 8 * S + 7);
        v0 = n0; v1 = n1; n0 = m0; n1 = m1;
        pv_step<S + 1, N, W0>(base, w, v0, v1, n0, n1, acc, hook);
    }
}
#undef RANGE_PV_MFMA

// steps 0..N-3 of a phase over the V rows at vslot, weights w[W0 ..]; s0/s1 = operands of steps 0 and
// 1 (already requested by the caller); steps N-2 and N-1 are returned in `carry`
template <int N, int W0, class Hook>
__device__ __forceinline__ void pv_steps(const float* vslot, const f32x4& w, PvOps s0, PvOps s1,
                                         f32x4 (&acc)[64], int lane, PvCarry& carry, Hook&& hook) {
    const float* base = vslot + (2 * (lane >> 4)) * VAL_DIM + 4 * (lane & 15);
    f32x4 v0 = s0.v0, v1 = s0.v1, n0 = s1.v0, n1 = s1.v1;
    pv_step<0, N, W0>(base, w, v0, v1, n0, n1, acc, hook);
    carry.v0a = v0; carry.v1a = v1; carry.v0b = n0; carry.v1b = n1;
    carry.w0 = w[W0 + N / 8 - 2]; carry.w1 = w[W0 + N / 8 - 1];
}

// MFMA results -> any non-MFMA reader: wait states first (hipcc pads nothing after an asm MFMA).
__device__ __forceinline__ void acc_fence(f32x4 (&acc)[64]) {
    asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");
#pragma unroll
    for (int i = 0; i < 64; i += 16)
        asm volatile("" : "+a"(acc[i]), "+a"(acc[i + 1]), "+a"(acc[i + 2]), "+a"(acc[i + 3]),
                          "+a"(acc[i + 4]), "+a"(acc[i + 5]), "+a"(acc[i + 6]), "+a"(acc[i + 7]),
                          "+a"(acc[i + 8]), "+a"(acc[i + 9]), "+a"(acc[i + 10]), "+a"(acc[i + 11]),
                          "+a"(acc[i + 12]), "+a"(acc[i + 13]), "+a"(acc[i + 14]), "+a"(acc[i + 15]));
}

// The finished accumulators of this wave's 16 queries -> their rows of the (64, 1024) tile at out_tile
// (queries past B are not written).  attend_stored_kernel's; attend_kernel keeps the same lines inline:
// through this function hipcc schedules its diagnostic variant's prologue differently.
__device__ __forceinline__ void store_acc_tile(f32x4 (&acc)[64], float* out_tile, int qt, int wave, int lane,
                                               int64_t B) {
    acc_fence(acc);
    // accumulator tile 4T+c, register r, lane (j,g)  ->  out[query 4g+r of this wave][64T + 4j + c]
    const int j = lane & 15, g = lane >> 4;
    const int64_t qw = (int64_t)qt * QTILE + wave * 16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t qo = qw + 4 * g + r;
        if (qo < B) {
            float* orow = out_tile + (wave * 16 + 4 * g + r) * VAL_DIM + 4 * j;
#pragma unroll
            for (int T = 0; T < 16; ++T) {
                f32x4 o = {acc[4 * T + 0][r], acc[4 * T + 1][r], acc[4 * T + 2][r], acc[4 * T + 3][r]};
                *reinterpret_cast<f32x4*>(orow + 64 * T) = o;
            }
        }
    }
}

// In front of carried steps whose weights hipcc may just have copied (v_mov) on the way in from another
// block: it pads nothing between a VALU write and an asm MFMA that reads the register.
__device__ __forceinline__ void carry_wait_states() { asm volatile("s_nop 1"); }

// the accumulators as opaque values in the AGPR file (no wait states: not behind an MFMA)
__device__ __forceinline__ void acc_pin(f32x4 (&acc)[64]) {
#pragma unroll
    for (int i = 0; i < 64; ++i) asm volatile("" : "+a"(acc[i]));
}

// Per-query constants of the combined weight: w = ca * 2^(k_sem*s - m1) + cb * 2^(k_geo*g - m2), from
// the global softmax statistics (m1, l1, m2, l2) of pass 1.  The pad queries of the last tile take the
// last real query's.  (Ordinary loads: pin_weight_consts puts hipcc's wait for them in front of the loop,
// see pin_qfrag.)
struct WeightConsts { float ca, cb, m1, m2; };
template <bool GEO>
__device__ __forceinline__ WeightConsts load_weight_consts(const ScanArgs& a, int64_t q) {
    const f32x4 st = *reinterpret_cast<const f32x4*>(a.stats + (q < a.B ? q : a.B - 1) * 4);
    WeightConsts k;
    k.m1 = st.x; k.m2 = st.z;
    k.ca = a.beta / st.y;
    k.cb = GEO ? (1.0f - a.beta) / st.w : 0.f;
    return k;
}
__device__ __forceinline__ void pin_weight_consts(WeightConsts& k) { asm volatile("" : "+v"(k.ca), "+v"(k.cb), "+v"(k.m1), "+v"(k.m2)); }

// The weights of one block from its logits (sem, geo: accumulator order), in one go: a segment's first
// block, in the prologue (every later block's are formed in slices between the PV MFMAs of the block
// before it), and the bf16-plane kernel's.  Pad rows are NOT masked here: attend_kernel and
// attend_bf16x3_kernel mask every block (zero_pad_rows), attend_stored_kernel zeroes only the last.
template <bool GEO>
__device__ __forceinline__ f32x4 block_weights(const WeightConsts& k, const ScanArgs& a, const f32x4& sem,
                                                     const f32x4& geo) {
    f32x4 w;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float wr = k.ca * __builtin_amdgcn_exp2f(fmaf(sem[r], a.k_sem, -k.m1));
        if (GEO) wr = fmaf(k.cb, __builtin_amdgcn_exp2f(fmaf(geo[r], a.k_geo, -k.m2)), wr);
        w[r] = wr;
    }
    return w;
}
// weight 0 for the rows of a block past its `valid` first ones (prow: this lane's rows, pi_row order)
__device__ __forceinline__ void zero_pad_rows(f32x4& w, const int (&prow)[4], int valid) {
#pragma unroll
    for (int r = 0; r < 4; ++r) w[r] = prow[r] < valid ? w[r] : 0.f;
}

// The segments of this workgroup (pass 2): one (split, query tile) item, or the walk of a stream-K
// range.  next() yields the query tile, its block range [b0, b1) and the (64, 1024) tile of the slab
// the partial goes to.  Everything here is wave-uniform (blockIdx only).
struct SegWalk {
    int64_t u, u_end;
    int split, col, cb0, cb;       // split-major: the item's split; stream-K: column, its first block / block count
    __device__ __forceinline__ void init(const ScanArgs& a) {
        col = -1;
        u = u_end = 0;
        cb0 = 0;
        cb = a.n_blocks;
        split = 0;
        if (a.sk_groups == 0) {
            int qt;
            decode_block(a, split, qt);
            const int b0 = part_begin(split, a.n_blocks, a.n_splits);
            const int b1 = part_begin(split + 1, a.n_blocks, a.n_splits);
            u = (int64_t)qt * a.n_blocks + b0;
            u_end = u + (b1 - b0);
        }
    }
    __device__ __forceinline__ bool next(const ScanArgs& a, int& qt, int& b0, int& b1, float*& out_tile) {
        if (a.sk_groups == 0) {
            if (u >= u_end) return false;
            qt = (int)(u / a.n_blocks);
            b0 = (int)(u - (int64_t)qt * a.n_blocks);
            b1 = b0 + (int)(u_end - u);
            out_tile = a.out + ((int64_t)split * a.B + (int64_t)qt * QTILE) * VAL_DIM;
            u = u_end;
            return true;
        }
        while (u >= u_end) {                       // next column
            if (++col >= a.sk_cols) return false;
            cb0 = sk_col_begin(col, a.n_blocks, a.sk_cols);
            cb = sk_col_begin(col + 1, a.n_blocks, a.sk_cols) - cb0;
            const int64_t U = (int64_t)a.n_qtiles * cb;
            u = sk_start(blockIdx.x, U, a.sk_groups);
            u_end = sk_start((int64_t)blockIdx.x + 1, U, a.sk_groups);
        }
        qt = (int)(u / cb);
        const int bo = (int)(u - (int64_t)qt * cb);
        const int64_t left = u_end - u;
        const int n = left < (int64_t)(cb - bo) ? (int)left : cb - bo;
        b0 = cb0 + bo;
        b1 = b0 + n;
        out_tile = a.out + ((int64_t)col * (a.sk_groups + a.n_qtiles) + blockIdx.x + qt) * (QTILE * VAL_DIM);
        u += n;
        return true;
    }
};

// LDS map (bytes): V ring 3 x 32 KB | K ring 2 x 16 KB | X ring 2 x 256 B  = 131,584 B
constexpr int ATTEND_LDS_BYTES = (3 * 8 * VAL_DIM + 2 * BLK * KEY_DIM + 2 * 64) * 4;

template <bool GEO, bool DIAG = false>
__global__ __launch_bounds__(256, 1) void attend_kernel(ScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* vring = reinterpret_cast<float*>(smem);          // 3 slots x [8][1024]
    // then K ring 2 slots x [16][256] and X ring 2 slots x [16][4]

    const uint32_t lds0 = (uint32_t)(uintptr_t)RANGE_LPTR(smem);
    const uint32_t vring_lds = lds0;
    const uint32_t kring_lds = lds0 + 3 * 8 * VAL_DIM * 4;
    const uint32_t xring_lds = kring_lds + 2 * BLK * KEY_DIM * 4;
    constexpr uint32_t VS_BYTES = 8 * VAL_DIM * 4, KT_BYTES = BLK * KEY_DIM * 4;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4;
    const int swz = lane ^ (4 * wave);
    SegWalk walk;
    walk.init(a);
    int qt, b0, b1;
    float* out_tile;
    for (bool first_seg = true; walk.next(a, qt, b0, b1, out_tile); first_seg = false) {
    // (a later segment re-uses the LDS rings: every wave must be done with the previous one)
    if (!first_seg) __syncthreads();
    const int nb = b1 - b0;
    const int64_t q = (int64_t)qt * QTILE + wave * 16 + (lane & 15);

    QFrag f;
    load_qfrag(f, a.ehat, a.xq, a.B, q, g);
    WeightConsts wc = load_weight_consts<GEO>(a, q);
    pin_qfrag(f);
    pin_weight_consts(wc);       // (behind pin_qfrag: the order in which hipcc waits for the query loads)

    f32x4 acc[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    KAddr kaddr;
    kaddr.init(lane);
    const char* kring_b = smem + 3 * 8 * VAL_DIM * 4;
    const char* xring_b = kring_b + 2 * BLK * KEY_DIM * 4;
    // per-lane bank row of accumulator register r, relative to the block, and the number of
    // valid rows from this split's first row on (pad rows of the last block get weight 0)
    int prow[4];
    uint32_t kvoff[4];   // per-lane source offsets of the 4 K rows this wave moves (swizzled)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        prow[r] = pi_row(4 * g + r);
        kvoff[r] = (uint32_t)((swz ^ r) << 4);
    }
    const int n_left = (int)(a.n_valid - (int64_t)b0 * BLK);

    // Schedule (per wave; "half" = 8 bank rows, two per 16-row block t):
    //   half 2t   : wait+barrier | PV rows 0-7 of block t            (+ issue V half 2t+2)
    //   half 2t+1 : wait+barrier | QK of block t+1 | PV rows 8-15    (+ issue V half 2t+3,
    //               K/X tile t+2; the weights of block t+1 are formed between the PV MFMAs)
    // LDS-DMA groups in issue order: ... E(t-1)=8 | O(t-1)=8+5 | E(t)=8 | O(t)=8+5 ...; the
    // wait before barrier 2t leaves O(t-1) in flight, the one before barrier 2t+1 leaves E(t).
    // V half h lives in ring slot h%3 (re-filled two halves after its last read), K/X tile t in
    // slot t&1.  The steady state is branch-free: past the split's last block the prefetches
    // re-read that block (clamped) into slots nobody reads any more, so every group has its full
    // count and the waits are constants.
    f32x4 w_cur = {0.f, 0.f, 0.f, 0.f};
    if (nb > 0) {
        const int64_t r0 = (int64_t)b0 * BLK;
        const int64_t r1 = (int64_t)(nb > 1 ? b0 + 1 : b0) * BLK;
        issue_k_tile(a.keys, a.xyz4, r0, kring_lds, xring_lds, wave, lane, swz);
        issue_v_half(a.values, r0, vring_lds, wave, lane);
        issue_v_half(a.values, r0 + 8, vring_lds + VS_BYTES, wave, lane);
        issue_k_tile(a.keys, a.xyz4, r1, kring_lds + KT_BYTES, xring_lds + 256, wave, lane, swz);
        RANGE_WAIT_BARRIER(21);
        QKAcc c;
        qk_mfma<GEO>(kring_b, qk_first_reads<GEO>(kring_b, xring_b, kaddr), kaddr, f, c,
                     [](int) __attribute__((always_inline)) {});
        c.fence();
        w_cur = block_weights<GEO>(wc, a, c.a0, c.g);
        zero_pad_rows(w_cur, prow, n_left);          // (this kernel masks every block as it forms its weights)
    }
    int vs = 0;   // V slot of half 2t
    PvCarry carry;
    carry.zero();
    unsigned long long d_vm0 = 0, d_bar0 = 0, d_pv0 = 0, d_vm1 = 0, d_bar1 = 0, d_qk = 0, d_pv1 = 0;
    unsigned long long d_mark = 0;
    const unsigned long long d_start = DIAG ? stamp() : 0;
    const int b_last = b1 - 1;
    for (int t = 0; t < nb; ++t) {
        const int vs1 = vs == 2 ? 0 : vs + 1;
        const int vs2 = vs1 == 2 ? 0 : vs1 + 1;
        const int bn1 = min(b0 + t + 1, b_last), bn2 = min(b0 + t + 2, b_last);
        // wave-uniform source / destination bases of this wave's pieces
        const float* vsrc1 = a.values + ((int64_t)bn1 * BLK + 2 * wave) * VAL_DIM;     // rows 2w, 2w+1
        const float* ksrc2 = a.keys + ((int64_t)bn2 * BLK + 4 * wave) * KEY_DIM;       // rows 4w..4w+3
        const float* xsrc2 = a.xyz4 + (int64_t)bn2 * BLK * 4;
        const uint32_t vdst_e = vring_lds + vs2 * VS_BYTES + wave * 8192;   // half 2t+2
        const uint32_t vdst_o = vring_lds + vs * VS_BYTES + wave * 8192;    // half 2t+3
        const uint32_t kdst = kring_lds + (t & 1) * KT_BYTES + wave * 4096;
        const uint32_t xdst = xring_lds + (t & 1) * 256;
        const uint32_t vvoff = (uint32_t)(lane << 4);
        // ---- half 2t
        RANGE_WB(13, d_vm0, d_bar0);
        if (DIAG) d_mark = stamp();
        {
            PvOps s0, s1;
            pv_first_reads(vring + vs * 8 * VAL_DIM, lane, s0, s1);
            pv_exec_carry(acc, carry);                       // last step of the previous half
            pv_steps<16, 0>(vring + vs * 8 * VAL_DIM, w_cur, s0, s1, acc, lane, carry,
                     [&](int h) __attribute__((always_inline)) {
                         if (h % 14 == 3) {                  // 8 pieces: V half 2t+2
                             const int ii = h / 14;
                             if ((ii & 3) == 0) dma_group_begin(vdst_e + (ii >> 2) * 4096);
                             dma_b128_q(vsrc1 + (ii >> 2) * VAL_DIM, vvoff, ii & 3);
                         }
                     });
        }
        // ---- half 2t+1
        if (DIAG) d_pv0 += stamp() - d_mark;
        RANGE_WB(8, d_vm1, d_bar1);
        if (DIAG) d_mark = stamp();
        QKAcc c;
        PvOps s0, s1;
        {
            const char* kt = kring_b + ((t + 1) & 1) * KT_BYTES;
            const KFirst kf = qk_first_reads<GEO>(kt, xring_b + ((t + 1) & 1) * 256, kaddr);
            pv_exec_carry(acc, carry);                       // last step of half 2t
            qk_mfma<GEO>(kt, kf, kaddr, f, c, [&](int s_) __attribute__((always_inline)) {
                if (s_ == 13) pv_first_reads(vring + vs1 * 8 * VAL_DIM, lane, s0, s1);
            });
        }
        if (DIAG) { const unsigned long long x_ = stamp(); d_qk += x_ - d_mark; d_mark = x_; }
        f32x4 w_next = {0.f, 0.f, 0.f, 0.f};
        float e1[4], e2[4];
        const int n_left1 = n_left - (t + 1) * BLK;
        pv_steps<16, 2>(vring + vs1 * 8 * VAL_DIM, w_cur, s0, s1, acc, lane, carry,
                [&](int h) __attribute__((always_inline)) {
                    if ((h & 7) == 3) {
                        const int ii = h >> 3;               // 13 pieces: V half 2t+3, K/X tile t+2
                        if (ii < 8) {
                            if ((ii & 3) == 0) dma_group_begin(vdst_o + (ii >> 2) * 4096);
                            dma_b128_q(vsrc1 + (8 + (ii >> 2)) * VAL_DIM, vvoff, ii & 3);
                        } else if (ii < 12) {
                            if (ii == 8) dma_group_begin(kdst);
                            dma_b128_q(ksrc2, kvoff[ii - 8], ii - 8);
                        } else if (ii == 12) {
                            dma_b32(xsrc2, (uint32_t)(lane << 2), xdst);
                        }
                    } else if (h >= 21 && h < 101 && ((h - 21) & 3) == 0) {
                        // weights of block t+1 in 20 slices of <= 4 VALU instructions; the first
                        // runs >= 20 MFMAs after the last QK MFMA, whose results are long readable
                        const int k = (h - 21) >> 2, r = k / 5, part = k % 5;
                        if (part == 0) {
                        } else if (part == 1) {
                            e1[r] = fmaf(c.a0[r], a.k_sem, -wc.m1);
                            if (GEO) e2[r] = fmaf(c.g[r], a.k_geo, -wc.m2);
                        } else if (part == 2) {
                            e1[r] = __builtin_amdgcn_exp2f(e1[r]);
                        } else if (part == 3) {
                            if (GEO) e2[r] = __builtin_amdgcn_exp2f(e2[r]);
                        } else {
                            float wr = wc.ca * e1[r];
                            if (GEO) wr = fmaf(wc.cb, e2[r], wr);
                            w_next[r] = prow[r] < n_left1 ? wr : 0.f;
                        }
                    }
                });
        if (DIAG) d_pv1 += stamp() - d_mark;
        w_cur = w_next;
        vs = vs2;
    }
    if (nb > 0) pv_exec_carry(acc, carry);   // last step of the last half
    // the clamped prefetches of the last iterations are still in flight into this workgroup's LDS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (DIAG && lane == 0 && a.diag) {
        unsigned long long* d = a.diag + ((size_t)blockIdx.x * 4 + wave) * 16;
        d[0] = d_vm0; d[1] = d_bar0; d[2] = d_pv0; d[3] = d_vm1; d[4] = d_bar1; d[5] = d_qk;
        d[6] = d_pv1; d[7] = stamp() - d_start; d[8] = (unsigned long long)nb; d[9] = d_start;
        unsigned xcc; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        d[10] = xcc & 0xf;
    }

    acc_fence(acc);
    // as store_acc_tile: tile 4T+c, register r, lane (j,g)  ->  out[query 4g+r of this wave][64T + 4j + c]
    const int j = lane & 15;
    const int64_t qw = (int64_t)qt * QTILE + wave * 16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t qo = qw + 4 * g + r;
        if (qo < a.B) {
            float* orow = out_tile + (wave * 16 + 4 * g + r) * VAL_DIM + 4 * j;
#pragma unroll
            for (int T = 0; T < 16; ++T) {
                f32x4 o = {acc[4 * T + 0][r], acc[4 * T + 1][r], acc[4 * T + 2][r], acc[4 * T + 3][r]};
                *reinterpret_cast<f32x4*>(orow + 64 * T) = o;
            }
        }
    }
    }   // segments
}

// ------------------------------------------------------------------------------------------------
// pass 2 on KEPT logits.  Same weight arithmetic and the same summation order per accumulator tile
// as attend_kernel (the outputs are bit-identical), but the semantic logits of block t+1 are not
// recomputed (64 of the 321 MFMAs per block and wave): pass 1 left them in HBM in accumulator
// order, and they arrive like a K tile did - one 1 KB LDS-DMA per wave and block into a 2-slot
// ring - at 4 B per (query, row) of extra HBM traffic each way, on a kernel that is MFMA-bound.
// The geographic tile (one MFMA per block) is still recomputed from the X ring.
//
// Without a K ring the LDS holds two WHOLE blocks of V, so the waves meet once per block, not once
// per half, and a block is one phase of 256 + 1 MFMAs (pv_steps<32>):
//   block t : wait(everything)+barrier | first LDS reads: S/X of block t+1, V steps 0-1 of block t
//             | the 2 carried steps of block t-1 | geo MFMA of block t+1
//             | PV rows 0-7   (+ issue S/X tile t+2, then the 16 V pieces of block t+1)
//             | PV rows 8-15  (+ the weights of block t+1, one VALU instruction per gap)
// V block t lives in ring slot t&1; S/X tile t in slot t&1.  The barrier at the top of block t
// covers landing (all of a wave's outstanding LDS-DMAs were issued in the FIRST half of block t-1:
// at least half a block of lead, so the wait is vmcnt(0)) and re-use (every wave has finished
// reading V block t-1 and S/X tile t, whose slots this block refills; the carried steps hold their
// operands in registers).  The block loop is unrolled by two, which makes every slot address a
// constant and w_cur / w_next two names.  Past the segment's last block the prefetches re-read
// that block (clamped) into slots nobody reads any more: the steady state is branch-free.
// LDS map (bytes): V ring 2 x 64 KB | S ring 2 x 4 KB (1 KB per wave) | X ring 2 x 256 B = 139,776 B
// LDS-DMA operations per wave and block: 1 S + 1 X + 16 V = 18.
// ------------------------------------------------------------------------------------------------
constexpr int ATTEND_STORED_LDS_BYTES = (2 * BLK * VAL_DIM + 2 * 1024 + 2 * 64) * 4;

template <int V> struct IntC { __device__ constexpr operator int() const { return V; } };

template <bool GEO>
__global__ __launch_bounds__(256, 1) void attend_stored_kernel(ScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* vring = reinterpret_cast<float*>(smem);          // 2 slots x [16][1024]
    constexpr uint32_t VB_BYTES = BLK * VAL_DIM * 4;
    const uint32_t lds0 = (uint32_t)(uintptr_t)RANGE_LPTR(smem);
    const uint32_t vring_lds = lds0;
    const uint32_t sring_lds = lds0 + 2 * VB_BYTES;
    const uint32_t xring_lds = sring_lds + 2 * 4096;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4;
    SegWalk walk;
    walk.init(a);
    int qt, b0, b1;
    float* out_tile;
    for (bool first_seg = true; walk.next(a, qt, b0, b1, out_tile); first_seg = false) {
    // (a later segment re-uses the LDS rings: every wave must be done with the previous one)
    if (!first_seg) __syncthreads();
    const int nb = b1 - b0;
    const int64_t q = (int64_t)qt * QTILE + wave * 16 + (lane & 15);
    const int64_t qtile_kept = (int64_t)qt + a.qt_offset;

    WeightConsts wc = load_weight_consts<GEO>(a, q);
    pin_weight_consts(wc);
    float fxq = a.xq[(q < a.B ? q : a.B - 1) * 4 + g];       // geo head of the query, as QFrag::xq
    asm volatile("" : "+v"(fxq));                            // (an ordinary load too: same pin)

    f32x4 acc[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    // (opaque zeros: as plain constants hipcc re-creates them in front of the odd tail, gives the tail
    // another register assignment than the loop and shuffles - and spills - the tiles between the two)
    acc_pin(acc);

    const char* sring_b = smem + 2 * VB_BYTES;
    const char* xring_b = sring_b + 2 * 4096;
    const uint32_t s_rd = (uint32_t)(wave * 1024 + lane * 16);                  // this lane's logits
    const uint32_t x_rd = (uint32_t)((pi_row(lane & 15) * 4 + g) * 4);          // as KAddr::x
    int prow[4];
    lane_rows(prow, g);
    const int n_left = (int)(a.n_valid - (int64_t)b0 * BLK);
    const uint32_t vvoff = (uint32_t)(lane << 4);

    // one S tile (this wave's 1 KB) + the X tile: 2 vector-memory operations per wave
    auto issue_sx = [&](int block, int slot) __attribute__((always_inline)) {
        dma_b128(a.logits + logit_tile(qtile_kept, a.n_blocks, block, wave), vvoff,
                 sring_lds + slot * 4096 + wave * 1024);
        dma_b32(a.xyz4 + (int64_t)block * BLK * 4, (uint32_t)(lane << 2), xring_lds + slot * 256);
    };

    f32x4 w_a = {0.f, 0.f, 0.f, 0.f}, w_b = {0.f, 0.f, 0.f, 0.f};
    if (nb > 0) {
        const int64_t r0 = (int64_t)b0 * BLK;
        issue_sx(b0, 0);
        issue_v_half(a.values, r0, vring_lds, wave, lane);
        issue_v_half(a.values, r0 + 8, vring_lds + VB_BYTES / 2, wave, lane);
        issue_sx(nb > 1 ? b0 + 1 : b0, 1);
        RANGE_WAIT_BARRIER(18);                             // S/X tile 0 has landed
        const f32x4 sv = *reinterpret_cast<const f32x4*>(sring_b + s_rd);
        f32x4 cg = {0.f, 0.f, 0.f, 0.f};
        if (GEO) {
            const float xa = *reinterpret_cast<const float*>(xring_b + x_rd);
            mfma_v_first(cg, xa, fxq);
            asm volatile("s_nop 15" : "+v"(cg));
        }
        w_a = block_weights<GEO>(wc, a, sv, cg);     // (pad rows: zeroed below, in front of the last block)
    }
    PvCarry carry;
    carry.zero();
    const int b_last = b1 - 1;

    // block t of the segment, in ring slot P = t & 1, with the weights w_cur; forms w_next (block t+1)
    auto run_block = [&](auto par, int t, const f32x4& w_cur, f32x4& w_next) __attribute__((always_inline)) {
        const int P = par;
        const int bn1 = min(b0 + t + 1, b_last), bn2 = min(b0 + t + 2, b_last);
        const float* vsrc1 = a.values + ((int64_t)bn1 * BLK + 2 * wave) * VAL_DIM;     // rows 2w, 2w+1 (+8)
        const float* ssrc2 = a.logits + logit_tile(qtile_kept, a.n_blocks, bn2, wave);
        const float* xsrc2 = a.xyz4 + (int64_t)bn2 * BLK * 4;
        const uint32_t vdst = vring_lds + (P ^ 1) * VB_BYTES + wave * 8192;     // block t+1
        const uint32_t sdst = sring_lds + P * 4096 + wave * 1024;               // tile t+2
        const uint32_t xdst = xring_lds + P * 256;
        const float* vslot = vring + P * BLK * VAL_DIM;
        RANGE_WAIT_BARRIER(0);
        PvOps s0, s1;
        f32x4 cg = {0.f, 0.f, 0.f, 0.f};
        const f32x4 sv = *reinterpret_cast<const f32x4*>(sring_b + (P ^ 1) * 4096 + s_rd);
        {
            const float xa = GEO ? *reinterpret_cast<const float*>(xring_b + (P ^ 1) * 256 + x_rd) : 0.f;
            pv_first_reads(vslot, lane, s0, s1);
            carry_wait_states();
            pv_exec_carry(acc, carry);                       // last 2 steps of block t-1
            if (GEO) mfma_v_first(cg, xa, fxq);
        }
        float e1[4], e2[4];
        pv_steps<32, 0>(vslot, w_cur, s0, s1, acc, lane, carry,
                [&](int h) __attribute__((always_inline)) {
                    if (h < 128) {
                        if (h % 6 == 3) {                    // 18 pieces: S/X tile t+2, V block t+1
                            const int ii = h / 6;
                            if (ii == 0) {
                                dma_b128(ssrc2, vvoff, sdst);
                            } else if (ii == 1) {
                                dma_b32(xsrc2, (uint32_t)(lane << 2), xdst);
                            } else if (ii < 18) {
                                const int p = ii - 2, hh = p >> 3, row = (p >> 2) & 1, qq = p & 3;
                                if (qq == 0) dma_group_begin(vdst + hh * (VB_BYTES / 2) + row * 4096);
                                dma_b128_q(vsrc1 + (8 * hh + row) * VAL_DIM, vvoff, qq);
                            }
                        }
                    } else if (h >= 150 && h < 206 && (h & 1) == 0) {
                        // weights of block t+1, ONE VALU instruction per MFMA gap (an exp2 is a
                        // quarter-rate instruction: two of them in one gap delay the next MFMA).
                        // The first runs > 140 MFMAs after the geo MFMA, whose result is long
                        // readable.
                        const int k = (h - 150) >> 1, r = k / 7, op = k % 7;
                        if (op == 0) e1[r] = fmaf(sv[r], a.k_sem, -wc.m1);
                        else if (op == 1) { if (GEO) e2[r] = fmaf(cg[r], a.k_geo, -wc.m2); }
                        else if (op == 2) e1[r] = __builtin_amdgcn_exp2f(e1[r]);
                        else if (op == 3) { if (GEO) e2[r] = __builtin_amdgcn_exp2f(e2[r]); }
                        else if (op == 4) e1[r] = valu_mul(wc.ca, e1[r]);
                        else if (op == 5) { if (GEO) e1[r] = valu_fma(wc.cb, e2[r], e1[r]); }
                        else w_next[r] = e1[r];
                    }
                });
    };

    if (nb > 0) {
        // pad rows exist only in the bank's last block, and that can only be a segment's last: their
        // weights are zeroed once, in front of that block
        const int valid_last = n_left - (nb - 1) * BLK;
        int t = 0;
        for (; t + 2 <= nb; t += 2) {
            run_block(IntC<0>{}, t, w_a, w_b);
            if (t + 2 == nb && valid_last < BLK) zero_pad_rows(w_b, prow, valid_last);
            run_block(IntC<1>{}, t + 1, w_b, w_a);
        }
        if (t < nb) {                                        // odd tail
            if (valid_last < BLK) zero_pad_rows(w_a, prow, valid_last);
            run_block(IntC<0>{}, t, w_a, w_b);
        }
        carry_wait_states();
        pv_exec_carry(acc, carry);                           // last 2 steps of the last block
    }
    // the clamped prefetches of the last blocks are still in flight into this workgroup's LDS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    store_acc_tile(acc, out_tile, qt, wave, lane, a.B);
    }   // segments
}


// Sum of the parts of float4 column c4 of query q: column by column, parts ascending (= ascending bank
// blocks), the first part assigned and not added to zero.  UNROLL loads are in flight; the additions
// keep their order.
template <int UNROLL>
__device__ __forceinline__ f32x4 sum_parts(const float* parts, const SlabMap& m, int64_t B, int64_t q, int c4) {
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int col = 0; col < slab_cols(m); ++col) {
        int64_t first4, stride4;
        int n;
        slab_parts(m, B, q, col, first4, stride4, n);
        const f32x4* p4 = reinterpret_cast<const f32x4*>(parts) + first4 + c4;
        if (col == 0) s = p4[0];
#pragma unroll UNROLL
        for (int p = col == 0 ? 1 : 0; p < n; ++p) s += p4[(int64_t)p * stride4];
    }
    return s;
}

// the parts of pass 2 (SlabMap) -> (B, 1024) f32, fixed summation order (ascending bank blocks).
__global__ void reduce_parts_kernel(const float* parts, SlabMap m, int64_t B, float* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * (VAL_DIM / 4)) return;
    const int64_t q = i / (VAL_DIM / 4);
    const int c4 = (int)(i - q * (VAL_DIM / 4));
    reinterpret_cast<f32x4*>(out)[i] = sum_parts<4>(parts, m, B, q, c4);
}

// out = (1-beta)*G + beta*H, elementwise f32, with the reference's rounding (two products, one
// sum, no FMA contraction): range/range.py:238.  Used by the beta sweep, where H (beta=1) and G
// (beta=0) are computed once and blended for every beta.
__global__ void blend_kernel(const float* G, const float* H, float beta, int64_t n4, float* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const f32x4 g = reinterpret_cast<const f32x4*>(G)[i];
    const f32x4 h = reinterpret_cast<const f32x4*>(H)[i];
    const float a = 1.0f - beta;
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = __fadd_rn(__fmul_rn(a, g[k]), __fmul_rn(beta, h[k]));
    reinterpret_cast<f32x4*>(out)[i] = o;
}

// out (B,1280) f64 = [ sum_p partial_p (f32, widened) | ehat64 ]      (range/range.py:222, :240)
// for queries [q0, q0 + nq) of a batch of B (parts: (n_parts,B,1024), ehat64 / out: (B,..)).
__global__ void finalize_kernel(const float* parts, SlabMap m, const double* ehat64, int64_t B,
                                int64_t q0, int64_t nq, double* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over nq * 320 quads
    if (i >= nq * 320) return;
    const int64_t q = q0 + i / 320;
    const int c = (int)(i % 320);
    double* o = out + q * 1280 + 4 * c;
    if (c < 256) {
        const f32x4 s = sum_parts<8>(parts, m, B, q, c);
        o[0] = (double)s.x; o[1] = (double)s.y; o[2] = (double)s.z; o[3] = (double)s.w;
    } else {
        const double* e = ehat64 + q * 256 + 4 * (c - 256);
        o[0] = e[0]; o[1] = e[1]; o[2] = e[2]; o[3] = e[3];
    }
}

}  // namespace range_hip
