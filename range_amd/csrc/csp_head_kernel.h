// The class head of the reference's CSP models (location_models/csp/main/models.py:135-173: class_emb, a
// Linear(num_filts, num_classes, bias = False), then a sigmoid): (B, num_filts) float32 embeddings in,
//   PROBS  : sigmoid(X W^T)           (B, M)
//   LOGITS : X W^T                    (B, M)   (eval_single_class)
//   SUM    : sum over ALL classes of the sigmoid   (B)
// out, as a launch of its own behind csp_kernel.h's (the embedding's round trip through HBM is 3 % of the
// (B, 8142) result's bytes).  host_plan.h: csp_head_plan.
//
// ARITHMETIC.  v_mfma_f32_32x32x2_f32 as the layers: exact float32 products, every output ONE k-ordered chain
// from 0.  An output's bits therefore depend on its row of X and its row of W alone - not on B, the row's
// place in a tile, the tile's place in the grid, or the columns computed beside it.
//
// TILE.  T = 64 rows of X (32 when num_filts > 512) in LDS, row stride `ld` odd (the 32 rows of an A operand
// fall into 32 banks), columns up to the padded K zero, rows beyond B zero.  A pass finishes `cols_per_pass`
// columns of the tile: column tile t of chunk ch goes to wave (t & 3), which holds its NT = CSP_HEAD_ACC_TILES /
// MT tiles in accumulators - 64 registers, so that two workgroups fit a CU and one's loads, sigmoids and
// stores run under the other's MFMAs.  Work items - a row tile with a few consecutive chunks, for SUM with all
// its chunks - are walked grid-stride; the X tile is loaded only when the row tile changes, as 16-byte loads
// where the rows are 16-byte aligned.
//
// COLUMNS.  Lane n of a column tile computes column c = 32 tile + n of the call, i.e. class id = ids[c] (or c
// without an id array; c beyond M - 1 repeats column M - 1 and is not stored), and gathers that class's 16-byte
// fragments from the packed class_emb by csp_packed_index of the id.  A subset - M = 1 included - thus runs
// the chain of the full head and returns its columns bit for bit.  Fragments are read up to four k groups
// ahead into a register ring, as csp_gemm does.
//
// SUM.  The workgroup that owns the row tile walks all chunks.  A lane adds the sigmoids of its columns in
// column order (float32), the 32 lanes of a row are folded by a fixed xor tree, the four waves' partial sums
// added in wave order by one thread a row: no atomics, the same bits at every B and grid.
//
// Stores are non-temporal (the result is never read back here): per accumulator register 32 lanes write 128
// consecutive bytes of one row.  A NaN row of X gives a NaN row of the result.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csp_kernel.h"
#include "host_plan.h"

namespace range_hip {

using range_host::CSP_HEAD_LOGITS;
using range_host::CSP_HEAD_PROBS;
using range_host::CSP_HEAD_SUM;
using range_host::CSP_HEAD_ACC_TILES;

struct CspHeadArgs {
    const float* x;          // (B, K) float32
    const float4* w4;        // packed class_emb (csp_pack_head)
    const int32_t* ids;      // (M) class ids, or null: column c is class c
    float* out;              // (B, M), or (B) for SUM
    int64_t B, n_items;
    int32_t K, k_groups, ld, M, col_tiles, n_chunks, num_classes, chunks_per_item, groups;
};

// acc[m][j] += X[32 m .. 32 m + 31][:] W[class of this lane in tile j][:], j < NTW.  base[j]: the float4 index of
// this lane's fragment of k group 0 (the lane's class, its k parity); the next k group is 64 further on.
template <int MT, int NT, int NTW>
__device__ __forceinline__ void csp_head_gemm(csp_f32x16 (&acc)[MT][NT], const float4* w4, const uint32_t (&base)[NT],
                                              int k_groups, const float* xa, int m_stride) {
    constexpr int D = NTW > 4 ? 2 : 4;
    float4 b[D][NTW];
    const int kg_last = k_groups - 1;
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
        for (int j = 0; j < NTW; ++j) b[d][j] = w4[base[j] + (uint32_t)(d < kg_last ? d : kg_last) * 64u];
    for (int kg0 = 0; kg0 < k_groups; kg0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int kg = kg0 + d;
            if (kg < k_groups) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    float av[MT];
#pragma unroll
                    for (int m = 0; m < MT; ++m) av[m] = xa[m * m_stride + kg * 8 + 2 * s];
#pragma unroll
                    for (int j = 0; j < NTW; ++j) {
                        const float bv = s == 0 ? b[d][j].x : s == 1 ? b[d][j].y : s == 2 ? b[d][j].z : b[d][j].w;
#pragma unroll
                        for (int m = 0; m < MT; ++m)
                            acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m], bv, acc[m][j], 0, 0, 0);
                    }
                }
            }
            const int kn = kg + D < kg_last ? kg + D : kg_last;
#pragma unroll
            for (int j = 0; j < NTW; ++j) b[d][j] = w4[base[j] + (uint32_t)kn * 64u];
        }
    }
}

template <int MT, int NT, int NTW = NT>
__device__ __forceinline__ void csp_head_gemm_dispatch(csp_f32x16 (&acc)[MT][NT], int ntw, const float4* w4,
                                                       const uint32_t (&base)[NT], int k_groups, const float* xa,
                                                       int m_stride) {
    if (ntw == NTW) csp_head_gemm<MT, NT, NTW>(acc, w4, base, k_groups, xa, m_stride);
    else if constexpr (NTW > 1) csp_head_gemm_dispatch<MT, NT, NTW - 1>(acc, ntw, w4, base, k_groups, xa, m_stride);
}

// The X tile: rows b0 .. b0 + T - 1 of x (B, K) into `hx`, row stride ld, columns K .. k_pad - 1 and rows beyond
// B zero.  Wave w loads rows w, w + 4, ...; a lane the columns lane, lane + 64, ... (16 bytes each where vec4:
// every row starts 16-byte aligned - K % 4 == 0: then k_pad % 4 == 0 and K..k_pad is whole float4s).
template <int T>
__device__ __forceinline__ void csp_head_load_x(const float* x, int64_t B, int64_t b0, int K, int k_pad, int ld, bool vec4,
                                                float* hx, int wave, int lane) {
    if (vec4) {
#pragma unroll 4
        for (int r = wave; r < T; r += 4) {
            const bool live = b0 + r < B;
            const float4* const src = reinterpret_cast<const float4*>(x + (b0 + r) * K);
            for (int k4 = lane; 4 * k4 < k_pad; k4 += 64) {
                const float4 v = live && 4 * k4 < K ? src[k4] : float4{0.0f, 0.0f, 0.0f, 0.0f};
                float* const dst = hx + r * ld + 4 * k4;
                dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
            }
        }
    } else {
#pragma unroll 4
        for (int r = wave; r < T; r += 4) {
            const bool live = b0 + r < B;
            for (int k = lane; k < k_pad; k += 64) hx[r * ld + k] = live && k < K ? x[(b0 + r) * K + k] : 0.0f;
        }
    }
}

// The columns of a wave's tiles t0, t0 + 4, ...: col[j] the lane's column of the call, base[j] the float4 index of
// its class's fragment of k group 0 in the packed class_emb (csp_packed_index of the id, the lane's k parity lh).
template <int NT>
__device__ __forceinline__ void csp_head_columns(uint32_t (&base)[NT], int (&col)[NT], int t0, int l31, int lh,
                                                 const int32_t* ids, int M, int num_classes, int k_groups) {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int c = (t0 + 4 * j) * 32 + l31;
        const int cc = c < M ? c : M - 1;
        int id = ids ? ids[cc] : cc;
        id = id < 0 ? 0 : id < num_classes ? id : num_classes - 1;     // (a bad device id reads class 0 / C - 1)
        col[j] = c;
        base[j] = ((uint32_t)(id >> 5) * (uint32_t)k_groups) * 64u + 32u * lh + (uint32_t)(id & 31);
    }
}

template <int MT, int MODE>
__global__ __launch_bounds__(CSP_BLOCK, 2) void csp_head_kernel(CspHeadArgs a) {
    constexpr int T = 32 * MT;                  // rows of a tile
    constexpr int NT = CSP_HEAD_ACC_TILES / MT; // column tiles of a wave
    extern __shared__ __attribute__((aligned(16))) float csp_hx[];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l31 = lane & 31, lh = lane >> 5;
    const int ld = a.ld, K = a.K, k_pad = a.k_groups * 8;
    float* const part = csp_hx + T * ld;        // SUM: (4 waves, T) partial row sums
    // 16-byte loads of X: every row starts 16-byte aligned
    const bool vec4 = K % 4 == 0 && reinterpret_cast<uintptr_t>(a.x) % 16 == 0;
    int64_t loaded = -1;
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const int64_t rt = item / a.groups;
        const int ch0 = (int)(item - rt * a.groups) * a.chunks_per_item;
        const int ch1 = ch0 + a.chunks_per_item < a.n_chunks ? ch0 + a.chunks_per_item : a.n_chunks;
        const int64_t b0 = rt * T;
        if (rt != loaded) {
            __syncthreads();                    // the last item's reads of the tile (and of `part`) are done
            csp_head_load_x<T>(a.x, a.B, b0, K, k_pad, ld, vec4, csp_hx, wave, lane);
            __syncthreads();
            loaded = rt;
        }
        float s[MT][16];
        if (MODE == CSP_HEAD_SUM) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) s[m][r] = 0.0f;
        }
        for (int ch = ch0; ch < ch1; ++ch) {
            // this wave's column tiles of the chunk: t0, t0 + 4, ...
            const int t0 = ch * 4 * NT + wave;
            int ntw = a.col_tiles > t0 ? (a.col_tiles - t0 + 3) / 4 : 0;
            ntw = ntw < NT ? ntw : NT;
            if (ntw == 0) continue;
            uint32_t base[NT];
            int col[NT];
            csp_head_columns<NT>(base, col, t0, l31, lh, a.ids, a.M, a.num_classes, a.k_groups);
            csp_f32x16 acc[MT][NT];
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[m][j][r] = 0.0f;
            csp_head_gemm_dispatch<MT, NT>(acc, ntw, a.w4, base, a.k_groups, csp_hx + l31 * ld + lh, 32 * ld);
            // element r of a lane is row (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column lane & 31 of its 32x32 tile
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                if (j < ntw && col[j] < a.M) {
#pragma unroll
                    for (int m = 0; m < MT; ++m)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float v = MODE == CSP_HEAD_LOGITS ? acc[m][j][r]
                                                                    : csp_activation<range_host::CSP_ACT_SIGMOID>(acc[m][j][r]);
                            if (MODE == CSP_HEAD_SUM) {
                                s[m][r] += v;
                            } else {
                                const int64_t row = b0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                                if (row < a.B) __builtin_nontemporal_store(v, a.out + row * a.M + col[j]);
                            }
                        }
                }
            }
        }
        if (MODE == CSP_HEAD_SUM) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float v = s[m][r];
#pragma unroll
                    for (int o = 1; o < 32; o <<= 1) v += __shfl_xor(v, o);
                    if (l31 == 0) part[wave * T + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh] = v;
                }
            __syncthreads();
            if (t < T && b0 + t < a.B) a.out[b0 + t] = ((part[t] + part[T + t]) + part[2 * T + t]) + part[3 * T + t];
        }
    }
}

}  // namespace range_hip
