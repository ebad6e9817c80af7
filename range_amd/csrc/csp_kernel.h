// The reference's CSP location encoders ('CSP', 'CSP_INat': location_models/csp/main/models.py:135-152 ->
// SpatialRelationEncoder.py 'gridcell' :128-165 / 'theory' :522-562 -> module.py:104-229) as ONE launch:
// (lon, lat) degrees in, (B, num_filts) float32 embeddings out.
//
// TILE.  A workgroup of 256 threads (4 waves) takes T = 64 locations (32 when a layer is wider than 512;
// host_plan.h: csp_plan) and walks the tiles grid-stride, every index 64-bit.  The tile's activations live
// in ONE LDS image of T rows x `ld` floats; `ld` is odd, so that the 32 rows the lanes of an MFMA A operand
// read fall into 32 different banks.
//
// FEATURES.  One work item per (location, frequency), as posenc_kernel.h: the angles, sines and cosines in
// float64 (the arguments reach thousands of radians: a float32 angle is wrong in its second digit there),
// formed by that file's device functions with its rounding rules, then rounded ONCE to float32
// (torch.FloatTensor(numpy float64)) into the row.  gridcell: [lon: (sin, cos) per frequency | lat: ...],
// theory: per frequency (sin, cos) of the three angles.  Columns up to the first layer's padded K are zero.
//
// LAYERS.  Y = act(X W^T + b) on v_mfma_f32_32x32x2_f32: exact float32 products, each output a k-ordered
// fmaf chain from 0 - so a row's bits do not depend on where in a tile, or in which tile, it sits.  A = X
// from LDS (lane l: row l & 31, k = l >> 5), B = W^T from the packed weights (host_plan.h:
// csp_packed_index), streamed from L2 as one 16-byte load per lane, n tile and 8 k, up to four groups ahead.  The
// n tiles of a layer are dealt round-robin to the 4 waves; a wave keeps its whole share of the output - up
// to 8 accumulator tiles, 128 registers - until every wave has read X for the last time, and only then (one
// barrier) the tile's image is overwritten IN PLACE: that is what lets 64 rows x 512 floats, 128 KiB, do
// with one image.  The epilogue on the accumulators: bias, activation, the skip connection (X read from
// the image before the barrier), zeros into the padding columns.  LayerNorm (torch's: biased variance, eps
// 1e-5 under the root, affine) then runs over the image rows, 256 / T lanes a row, float32, two passes (mean,
// then squared deviations), over the layer's TRUE width only.  The last layer stores act(.) from the
// accumulators straight to `out`.
//
// NaN / infinite coordinates make their row NaN (sin(inf)), as in the reference; relu keeps a NaN (torch's
// does; fmaxf would not).  Rows of the last tile beyond B compute on zero features and are not stored.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_plan.h"
#include "posenc_kernel.h"

namespace range_hip {

using range_host::CSP_BLOCK;
using range_host::CSP_ACC_TILES;

typedef float csp_f32x16 __attribute__((ext_vector_type(16)));

struct CspLayerArgs {
    int32_t n, n_tiles, k_groups;    // true output width, its 32-column tiles, the input's groups of 8 k
    int32_t skip, layn;
    uint32_t w_off, b_off, g_off, be_off;   // floats into `params`
};

struct CspArgs {
    const double* freq;      // (F) float64, device
    const double* lonlat;    // (B,2) float64, (lon,lat) degrees
    const float* params;     // packed weights, biases, LayerNorm gamma / beta (csp_pack_layer)
    float* out;              // (B, num_filts) float32
    int64_t B, n_tiles;
    const CspLayerArgs* layer;   // (n_layers), device
    int32_t F, kind, n_layers, ld, in0, in0_pad;
};

template <int ACT>
__device__ __forceinline__ float csp_activation(float v) {
    switch (ACT) {
        case range_host::CSP_ACT_SIGMOID: return 1.0f / (1.0f + expf(-v));
        case range_host::CSP_ACT_RELU: return v < 0.0f ? 0.0f : v;              // NaN stays NaN
        case range_host::CSP_ACT_LEAKYRELU: return v > 0.0f ? v : v * 0.2f;
        case range_host::CSP_ACT_TANH: return tanhf(v);
        default: return v * 0.5f * (1.0f + erff(v * 0.70710678118654752440f));  // nn.GELU(): the erf form
    }
}

// acc[m][j] += X[32 m .. 32 m + 31][:] W^T[:][n tile wave + 4 j], j < NTW: the k loop of one layer for a wave
// that owns NTW n tiles.  w4: the layer's packed weights, fragment (n tile, k group) = 64 lanes x 16 bytes.  The
// fragments are read D k groups ahead into a register ring (one wave a SIMD: nothing else hides the L2
// latency, and one group is only 4 MT NTW MFMAs = 0.4 us of work at NTW = 2); a slot is refilled right behind
// the MFMAs that read it, with the last group again where the layer ends (in bounds, unused).  xa: this lane's
// A element of k = 0 (row lane & 31, column lane >> 5), m_stride floats to the next 32 rows.
template <int MT, int NT, int NTW>
__device__ __forceinline__ void csp_gemm(csp_f32x16 (&acc)[MT][NT], const float4* w4, int k_groups, int wave, int lane,
                                         const float* xa, int m_stride) {
    constexpr int D = NTW > 4 ? 2 : 4;
    float4 b[D][NTW];
    const int kg_last = k_groups - 1;
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
        for (int j = 0; j < NTW; ++j) b[d][j] = w4[((size_t)(wave + 4 * j) * k_groups + (d < kg_last ? d : kg_last)) * 64 + lane];
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
            for (int j = 0; j < NTW; ++j) b[d][j] = w4[((size_t)(wave + 4 * j) * k_groups + kn) * 64 + lane];
        }
    }
}

template <int MT, int NT, int NTW = NT>
__device__ __forceinline__ void csp_gemm_dispatch(csp_f32x16 (&acc)[MT][NT], int ntw, const float4* w4, int k_groups,
                                                  int wave, int lane, const float* xa, int m_stride) {
    if (ntw == NTW) csp_gemm<MT, NT, NTW>(acc, w4, k_groups, wave, lane, xa, m_stride);
    else if constexpr (NTW > 1) csp_gemm_dispatch<MT, NT, NTW - 1>(acc, ntw, w4, k_groups, wave, lane, xa, m_stride);
}

template <int MT, int ACT>
__global__ __launch_bounds__(CSP_BLOCK) void csp_encode_kernel(CspArgs a) {
    constexpr int T = 32 * MT;                  // rows of a tile
    constexpr int NT = CSP_ACC_TILES / MT;      // n tiles of a wave
    constexpr int LPR = CSP_BLOCK / T;          // lanes per row in LayerNorm
    extern __shared__ __attribute__((aligned(16))) float csp_x[];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);     // (uniform: the n tiles of a wave are)
    const int l31 = lane & 31, lh = lane >> 5;
    const int ld = a.ld, F = a.F;
    for (int64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * T;
        // ---- features: float64 sines and cosines, rounded once to float32
        for (int item = t; item < T * F; item += CSP_BLOCK) {
            const int r = item / F, i = item - r * F;
            float* const row = csp_x + r * ld;
            const bool live = b0 + r < a.B;
            double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (live) {
                const double x = a.lonlat[2 * (b0 + r)], y = a.lonlat[2 * (b0 + r) + 1];
                const double f = a.freq[i];
                if (a.kind == PE_THEORY) posenc_theory_item(x, y, f, v);
                else posenc_lonlat_item(x, y, f, v[0], v[1], v[2], v[3]);
            }
            if (a.kind == PE_THEORY) {
#pragma unroll
                for (int j = 0; j < 6; ++j) row[6 * i + j] = (float)v[j];
            } else {
                row[2 * i] = (float)v[0];
                row[2 * i + 1] = (float)v[1];
                row[2 * F + 2 * i] = (float)v[2];
                row[2 * F + 2 * i + 1] = (float)v[3];
            }
        }
        const int pad0 = a.in0_pad - a.in0;
        for (int idx = t; idx < T * pad0; idx += CSP_BLOCK) {
            const int r = idx / pad0;
            csp_x[r * ld + a.in0 + (idx - r * pad0)] = 0.0f;
        }
        __syncthreads();
        for (int li = 0; li < a.n_layers; ++li) {
            const CspLayerArgs L = a.layer[li];
            const bool last = li + 1 == a.n_layers;
            // this wave's n tiles: wave, wave + 4, ...
            const int ntw = L.n_tiles > wave ? (L.n_tiles - wave + 3) / 4 : 0;
            csp_f32x16 acc[MT][NT];
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[m][j][r] = 0.0f;
            csp_gemm_dispatch<MT, NT>(acc, ntw, reinterpret_cast<const float4*>(a.params + L.w_off), L.k_groups, wave, lane,
                                      csp_x + l31 * ld + lh, 32 * ld);
            // ---- epilogue on the accumulators: element r of a lane is row (r & 3) + 8 (r >> 2) + 4 (lane >> 5),
            // column lane & 31 of its 32x32 tile
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                if (j < ntw) {
                    const int col = (wave + 4 * j) * 32 + l31;
                    const float bias = a.params[L.b_off + col];
#pragma unroll
                    for (int m = 0; m < MT; ++m)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int row = m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                            float v = csp_activation<ACT>(acc[m][j][r] + bias);
                            if (L.skip) v += csp_x[row * ld + col];
                            if (last) {
                                if (col < L.n && b0 + row < a.B) a.out[(b0 + row) * L.n + col] = v;
                            } else {
                                acc[m][j][r] = col < L.n ? v : 0.0f;
                            }
                        }
                }
            }
            __syncthreads();          // every wave has read X for the last time
            if (last) break;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                if (j < ntw) {
                    const int col = (wave + 4 * j) * 32 + l31;
#pragma unroll
                    for (int m = 0; m < MT; ++m)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            csp_x[(m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * ld + col] = acc[m][j][r];
                }
            }
            __syncthreads();
            if (L.layn) {
                // row t / LPR, columns q, q + LPR, ... of the TRUE width; the LPR lanes of a row are neighbours
                float* const row = csp_x + (t / LPR) * ld;
                const int q = t % LPR;
                const float inv_n = 1.0f / (float)L.n;
                float s = 0.0f;
                for (int c = q; c < L.n; c += LPR) s += row[c];
#pragma unroll
                for (int o = 1; o < LPR; o <<= 1) s += __shfl_xor(s, o);
                const float mean = s * inv_n;
                float d2 = 0.0f;
                for (int c = q; c < L.n; c += LPR) { const float d = row[c] - mean; d2 = fmaf(d, d, d2); }
#pragma unroll
                for (int o = 1; o < LPR; o <<= 1) d2 += __shfl_xor(d2, o);
                const float rstd = 1.0f / sqrtf(d2 * inv_n + 1e-5f);
                const float* const g = a.params + L.g_off;
                const float* const be = a.params + L.be_off;
                for (int c = q; c < L.n; c += LPR) row[c] = (row[c] - mean) * rstd * g[c] + be[c];
                __syncthreads();
            }
        }
    }
}

}  // namespace range_hip
