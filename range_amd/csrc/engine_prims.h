// Primitives every kernel header of the RANGE engine builds on: tile constants, the packed 16-bit
// conversions and bf16 planes, the inline-asm MFMA / LDS-DMA statements with the hazards each guards
// against, lane swaps, the merge of two statistics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_plan.h"

namespace range_hip {

using range_host::part_begin;       // (host_plan.h: the partition arithmetic, also run under sanitizers on the CPU)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int KEY_DIM = 256;
constexpr int VAL_DIM = 1024;
constexpr int QTILE = 64;        // queries per workgroup
constexpr int BLK = 16;          // bank rows per block
constexpr int MAX_TOPK = 16;
constexpr float NEG_BIG = -1.0e30f;

#define RANGE_LPTR(p) ((__attribute__((address_space(3))) void*)(p))

// MFMA row index i (0..15) of the transposed logit tile -> bank row inside the 16-row block.
// With i = 4g + r (g = lane group that will hold it, r = accumulator register):
//   row = 8*(r>>1) + 2*g + (r&1)
// so registers r=0,1 of every lane group cover the first 8-row half of the block and r=2,3 the
// second: the w @ V product can consume V in 8-row (32 KB) LDS slots.
__device__ __forceinline__ int pi_row(int i) { return ((i & 2) << 2) | ((i >> 2) << 1) | (i & 1); }
// the bank rows (inside a block) behind the 4 accumulator registers of a lane of group g
template <class T>
__device__ __forceinline__ void lane_rows(T (&prow)[4], int g) {
#pragma unroll
    for (int r = 0; r < 4; ++r) prow[r] = (T)pi_row(4 * g + r);
}

// round-to-nearest-even float32 -> bf16 of two values, packed (lo = a, hi = b)
__device__ __forceinline__ uint32_t cvt_pk_bf16(float a, float b) {
    uint32_t r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// two floats -> packed fp16, round to nearest even: gfx950's v_cvt_pk_f16_f32 (bitwise the (_Float16) cast
// on 2^24 pairs incl. exact ties and subnormal results: tools/micro/cvt_pk_f16_rne.hip)
__device__ __forceinline__ uint32_t cvt_pk_f16(float a, float b) {
    uint32_t r;
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// the two leading bf16 planes of a pair of floats, packed like cvt_pk_bf16 (x = x_h + x_m to 2^-17),
// and what the two leave (ra, rb)
__device__ __forceinline__ void split2(float a, float b, uint32_t& h, uint32_t& m, float& ra, float& rb) {
    h = cvt_pk_bf16(a, b);
    const float ha = a - __uint_as_float(h << 16), hb = b - __uint_as_float(h & 0xFFFF0000u);
    m = cvt_pk_bf16(ha, hb);
    ra = ha - __uint_as_float(m << 16);
    rb = hb - __uint_as_float(m & 0xFFFF0000u);
}

// f32 MFMA with the accumulator pinned to arch VGPRs (inline asm).  Why not the builtin: with a
// 512-register budget hipcc (ROCm 7.2) selects every builtin MFMA in its AGPR form; pass 2 already
// fills all 256 AGPRs with the output accumulators, and any further AGPR-form accumulator makes
// the allocator shuttle ~1000 registers per block through v_accvgpr_read/write.  The logit tile
// therefore accumulates in VGPRs through these statements.  hipcc pads nothing around an asm
// MFMA: the operands here come from LDS reads and long-lived registers (never a just-executed
// VALU write; the first MFMA of a chain still carries `s_nop 1`), and a chain ends with
// QKAcc::fence() before any non-MFMA instruction may read the results.
//
// WAR hazard on the A/B operands (measured on gfx950, tools/check_mfma_war.py): the compiler
// treats an asm statement's inputs as dead once the statement has issued and may give their
// registers to the very next VALU instruction; an MFMA is still reading them then, and the
// product comes out wrong (deterministically).  One wait state after the MFMA was enough in every
// experiment; each asm MFMA below carries a trailing `s_nop 1` (two), and tests/test_host_cpu.py checks the
// generated code for MFMA sources written by the following instruction.
__device__ __forceinline__ void mfma_v_first(f32x4& d, float a, float b) {
    asm volatile("s_nop 1\n\tv_mfma_f32_16x16x4_f32 %0, %1, %2, 0\n\ts_nop 1" : "=&v"(d) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma_v(f32x4& d, float a, float b) {
    asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0\n\ts_nop 1" : "+v"(d) : "v"(a), "v"(b));
}
// (8-pass MFMA result -> VALU read needs 11 wait states: QKAcc::fence gives 16.)

// ---- LDS-DMA (global_load_lds) by inline asm -------------------------------------------------
// The builtin form makes hipcc (ROCm 7.2) drain vmcnt(0) before the next LDS read because it
// cannot tell which LDS bytes the DMA writes; that would serialise the whole ring.  In asm the
// compiler neither counts nor waits for these operations: every wait on them below is a
// hand-counted s_waitcnt vmcnt(N) followed by a workgroup barrier.  M0 carries the wave-uniform
// LDS destination and is written inside the statement that uses it.  It is not restored: nothing
// else in these kernels uses M0 (gfx9+ DS instructions do not need it, no other LDS-DMA, movrel,
// GWS or sendmsg), and every statement that needs it sets it.
// sbase must be wave-uniform (SGPR pair), voff is the per-lane byte offset.
__device__ __forceinline__ void dma_b128(const void* sbase, uint32_t voff, uint32_t lds_addr) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %2"
                 :: "v"(voff), "s"(lds_addr), "s"(sbase) : "memory");
}
// (non-temporal cache policy: data streamed once per launch)
__device__ __forceinline__ void dma_b128_nt(const void* sbase, uint32_t voff, uint32_t lds_addr) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %2 nt"
                 :: "v"(voff), "s"(lds_addr), "s"(sbase) : "memory");
}
// Group form: the instruction's immediate offset is applied to BOTH the global and the LDS
// address, so a run of pieces that is contiguous in both spaces (the 4 quarter rows of a V row,
// the 4 rows of a K tile) needs M0 and the SGPR base only once.  dma_group_begin sets M0;
// dma_b128_q(q) issues piece q (byte offset q*1024, q = 0..3) relative to it.  M0 must survive
// between the statements of a group: nothing else in these kernels writes M0 (checked on the
// generated code by tests/test_host_cpu.py::test_no_foreign_m0_writes).
__device__ __forceinline__ void dma_group_begin(uint32_t lds_addr) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" :: "s"(lds_addr) : "memory");
}
__device__ __forceinline__ void dma_b128_q(const void* sbase, uint32_t voff, int q) {
    switch (q) {
        case 0: asm volatile("global_load_lds_dwordx4 %0, %1" :: "v"(voff), "s"(sbase) : "memory"); break;
        case 1: asm volatile("global_load_lds_dwordx4 %0, %1 offset:1024" :: "v"(voff), "s"(sbase) : "memory"); break;
        case 2: asm volatile("global_load_lds_dwordx4 %0, %1 offset:2048" :: "v"(voff), "s"(sbase) : "memory"); break;
        default: asm volatile("global_load_lds_dwordx4 %0, %1 offset:3072" :: "v"(voff), "s"(sbase) : "memory"); break;
    }
}
// the same with the non-temporal cache policy (streamed-once data: the key scan of a single pass)
__device__ __forceinline__ void dma_b128_q_nt(const void* sbase, uint32_t voff, int q) {
    switch (q) {
        case 0: asm volatile("global_load_lds_dwordx4 %0, %1 nt" :: "v"(voff), "s"(sbase) : "memory"); break;
        case 1: asm volatile("global_load_lds_dwordx4 %0, %1 offset:1024 nt" :: "v"(voff), "s"(sbase) : "memory"); break;
        case 2: asm volatile("global_load_lds_dwordx4 %0, %1 offset:2048 nt" :: "v"(voff), "s"(sbase) : "memory"); break;
        default: asm volatile("global_load_lds_dwordx4 %0, %1 offset:3072 nt" :: "v"(voff), "s"(sbase) : "memory"); break;
    }
}
__device__ __forceinline__ void dma_b32(const void* sbase, uint32_t voff, uint32_t lds_addr) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, %2"
                 :: "v"(voff), "s"(lds_addr), "s"(sbase) : "memory");
}

// wait for all but the n youngest vector-memory operations of this wave, then workgroup barrier.
// One asm statement with a memory clobber: no LDS access may be moved across it by the compiler.
#define RANGE_WAIT_BARRIER(n) asm volatile("s_waitcnt vmcnt(" #n ") lgkmcnt(0)\n\ts_barrier" ::: "memory")

__device__ __forceinline__ void merge_ml(float& m, float& l, float m2, float l2) {
    const float mm = fmaxf(m, m2);
    l = l * __builtin_amdgcn_exp2f(m - mm) + l2 * __builtin_amdgcn_exp2f(m2 - mm);
    m = mm;
}

// The value lane ^ 16 / lane ^ 32 holds, through gfx950's row-swap instructions instead of the LDS
// crossbar (ds_bpermute: ~120 cycles a round trip, and a wave alone on its SIMD has nothing to put
// into that time): v_permlane16_swap swaps the odd 16-lane rows of its first operand with the even
// rows of the second, v_permlane32_swap the upper half of the first with the lower half of the
// second.  With both operands = x the partner's value ends up in the second operand for lanes of
// even rows / the lower half and in the first for the others: one move, one swap, one select.
typedef uint32_t range_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t lane_xor16(uint32_t x) {
    const range_u32x2 r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
    return (__lane_id() & 16) ? r[0] : r[1];
}
__device__ __forceinline__ uint32_t lane_xor32(uint32_t x) {
    const range_u32x2 r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    return (__lane_id() & 32) ? r[0] : r[1];
}
__device__ __forceinline__ float lane_xor16(float x) { return __uint_as_float(lane_xor16(__float_as_uint(x))); }
__device__ __forceinline__ float lane_xor32(float x) { return __uint_as_float(lane_xor32(__float_as_uint(x))); }

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long x, int m) {
    const uint32_t lo = __shfl_xor((uint32_t)x, m), hi = __shfl_xor((uint32_t)(x >> 32), m);
    return ((unsigned long long)hi << 32) | lo;
}
template <int M>
__device__ __forceinline__ unsigned long long lane_xor_u64(unsigned long long x) {
    static_assert(M == 16 || M == 32, "row swaps exist for lane ^ 16 and lane ^ 32");
    const uint32_t lo = M == 16 ? lane_xor16((uint32_t)x) : lane_xor32((uint32_t)x);
    const uint32_t hi = M == 16 ? lane_xor16((uint32_t)(x >> 32)) : lane_xor32((uint32_t)(x >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// Output accumulators live in the 256 AGPRs for the whole kernel ("+a"): written as asm for the
// same reason as mfma_v - the builtin lets hipcc migrate accumulator tiles between the AGPR and
// VGPR halves of the register file inside the loop.
__device__ __forceinline__ void mfma_a(f32x4& acc, float a, float b) {
    asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0\n\ts_nop 1" : "+a"(acc) : "v"(a), "v"(b));
}

// The two scalings of a kept-logit weight (w = ca * e1 + cb * e2) as ONE scalar-float VALU
// instruction each.  Written as C++, hipcc's SLP vectoriser packs the products of neighbouring rows
// into v_pk_mul_f32 / v_pk_fma_f32 - and a packed float32 instruction beside MFMAs costs more MFMA
// issue time than the two scalar ones it replaces.  The packed forms round each
// lane like these, so the bits are the same.
__device__ __forceinline__ float valu_mul(float a, float b) {
    float d;
    asm volatile("v_mul_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
__device__ __forceinline__ float valu_fma(float a, float b, float c) {
    float d;
    asm volatile("v_fma_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}

}  // namespace range_hip
