// The fit of a whole CSP location encoder with its class head (include/range_cspfit.h; host_plan.h: cspfit_plan):
// one step of the reference's supervised stage (csp/main/trainer.py:753-797 -> trainer_helper.py:113-174:
// losses.py:395-470 embedding_loss without 'user', under torch.optim.Adam) with gradients through every layer of
// the feed-forward net (module.py:104-132), float32 as torch computes it in train mode.
//
// FORWARD.  cspfit_features_kernel writes the step's rows - B locations picked by an id array, then the Bg
// background locations - as the (R, in0) float32 features csp_kernel.h forms (posenc_kernel.h's items in float64,
// rounded once).  Per layer the product X W^T is csp_head_kernel's LOGITS launch over the layer's weight in the
// head's packed layout: every entry one k-ordered chain from 0, the chain of csp_encode_kernel.  cspfit_fwd_row_kernel
// then adds the bias IN PLACE (the saved pre-activation Z), applies activation, dropout and skip and, behind a
// LayerNorm, normalises the row with csp_encode_kernel's reductions (lpr lanes a row, column q, q + lpr, ..., a
// fixed xor tree): the embeddings of a fit are the bits range_csp_encode returns for the same network.
//
// DROPOUT.  keep(row, column) = (mix(mix(key ^ row) ^ column) >> 8) < floor((1 - p) 2^24), mix = the 32-bit
// finaliser below, key = the host's mix of (seed, step, layer): stateless, so the mask depends on nothing but
// those five numbers.  Kept entries are scaled by 1 / (1 - p).  p = 0 multiplies nothing.
//
// HEAD.  headfit_kernels.h's launches on the embeddings; behind every panel's logit gradient cspfit_back_kernel
// continues dE = G W_c (one chain ordered by class index, the accumulator re-read between panels).
//
// BACKWARD, per layer from the last.  cspfit_bwd_row_kernel recomputes the row's S = dropout(act(Z)) + X and its
// LayerNorm statistics from the saved Z and X in the forward's order and forms dS (the three-term formula), dZ =
// dS * mask * act'(Z) and dY * xhat.  cspfit_colsum_kernel adds the columns of dZ / dY * xhat / dY over the rows in
// row order (db, dgamma, dbeta), Adam behind it.  cspfit_back_kernel: dX = dZ W on v_mfma_f32_32x32x2_f32, A[m =
// row][k = output column] from dZ, B[k][n = input column] gathered from the packed W, one chain ordered by output
// column, the skip's dS added behind the chain.  dW = dZ^T X is headfit_update_kernel with G -> dZ.
//
// No atomics; no result depends on the grid, the stream or the class-panel width.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "headfit_kernels.h"
#include "host_plan.h"
#include "posenc_kernel.h"

namespace range_hip {

// (also on the host: cspfit_host.h derives the per-layer dropout keys with it)
__host__ __device__ __forceinline__ uint32_t cspfit_mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// the factor of dropout on entry (row, col): 1 / (1 - p) or 0
__device__ __forceinline__ float cspfit_drop(uint32_t key, uint32_t thresh, float scale, uint32_t row, uint32_t col) {
    return (cspfit_mix(cspfit_mix(key ^ row) ^ col) >> 8) < thresh ? scale : 0.0f;
}

__global__ __launch_bounds__(CSP_BLOCK) void cspfit_features_kernel(const double* freq, const double* lonlat, int64_t N,
                                                                    const int32_t* rows, int32_t B, const double* bg, int32_t R,
                                                                    int32_t F, int32_t kind, int32_t in0, float* x) {
    const int64_t total = (int64_t)R * F;
    for (int64_t item = (int64_t)blockIdx.x * CSP_BLOCK + threadIdx.x; item < total; item += (int64_t)gridDim.x * CSP_BLOCK) {
        const int32_t r = (int32_t)(item / F), i = (int32_t)(item - (int64_t)r * F);
        double lon, lat;
        if (r < B) {
            int64_t id = rows ? (int64_t)rows[r] : (int64_t)r;
            id = id < 0 ? 0 : id < N ? id : N - 1;
            lon = lonlat[2 * id]; lat = lonlat[2 * id + 1];
        } else {
            lon = bg[2 * (int64_t)(r - B)]; lat = bg[2 * (int64_t)(r - B) + 1];
        }
        const double f = freq[i];
        float* const row = x + (int64_t)r * in0;
        if (kind == PE_THEORY) {
            double v[6];
            posenc_theory_item(lon, lat, f, v);
#pragma unroll
            for (int j = 0; j < 6; ++j) row[6 * i + j] = (float)v[j];
        } else {
            double v0, v1, v2, v3;
            posenc_lonlat_item(lon, lat, f, v0, v1, v2, v3);
            row[2 * i] = (float)v0;
            row[2 * i + 1] = (float)v1;
            row[2 * F + 2 * i] = (float)v2;
            row[2 * F + 2 * i + 1] = (float)v3;
        }
    }
}

struct CspfitRowArgs {
    float* z;               // (R, n) forward: X W^T in, Z = X W^T + b out; backward: Z
    const float* xin;       // (R, n) the layer's input where its skip is live, else null
    float* y;               // forward: (R, n) the layer's output
    const float* dy;        // backward: (R, n) the gradient of the layer's output
    float* dz;              // backward: (R, n) dZ
    float* ds;              // backward: (R, n) dS, where the skip is live (else null)
    float* dyx;             // backward: (R, n) dY * xhat, behind a LayerNorm (else null)
    const float* bias; const float* gamma; const float* beta;   // gamma null: no LayerNorm
    int32_t R, n, lpr, drop_on;
    uint32_t drop_key, drop_thresh;
    float drop_scale;
};

// d act / d z at the pre-activation, as torch's backward kernels form it
template <int ACT>
__device__ __forceinline__ float cspfit_act_prime(float z) {
    switch (ACT) {
        case range_host::CSP_ACT_SIGMOID: { const float p = csp_activation<ACT>(z); return p * (1.0f - p); }
        case range_host::CSP_ACT_RELU: return z <= 0.0f ? 0.0f : 1.0f;           // (a NaN passes, as threshold_backward)
        case range_host::CSP_ACT_LEAKYRELU: return z > 0.0f ? 1.0f : 0.2f;
        case range_host::CSP_ACT_TANH: { const float t = tanhf(z); return 1.0f - t * t; }
        default: {
            const float cdf = 0.5f * (1.0f + erff(z * 0.70710678118654752440f));
            const float pdf = expf(-0.5f * z * z) * 0.39894228040143267794f;
            return cdf + z * pdf;
        }
    }
}

template <int ACT>
__global__ __launch_bounds__(CSP_BLOCK) void cspfit_fwd_row_kernel(CspfitRowArgs a) {
    const int t = threadIdx.x, lpr = a.lpr, rpw = CSP_BLOCK / lpr, q = t % lpr, n = a.n;
    const int64_t groups = ((int64_t)a.R + rpw - 1) / rpw;
    for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int64_t r = grp * rpw + t / lpr;
        if (r >= a.R) continue;                             // (the lpr lanes of a row leave together)
        float* const zr = a.z + r * n;
        float* const row = a.y + r * n;
        const float* const xr = a.xin ? a.xin + r * n : nullptr;
        float s = 0.0f;
        for (int c = q; c < n; c += lpr) {
            const float z = zr[c] + a.bias[c];
            float v = csp_activation<ACT>(z);
            if (a.drop_on) v *= cspfit_drop(a.drop_key, a.drop_thresh, a.drop_scale, (uint32_t)r, (uint32_t)c);
            if (xr) v += xr[c];
            zr[c] = z;
            row[c] = v;
            s += v;
        }
        if (!a.gamma) continue;
        const float inv_n = 1.0f / (float)n;
        for (int o = 1; o < lpr; o <<= 1) s += __shfl_xor(s, o);
        const float mean = s * inv_n;
        float d2 = 0.0f;
        for (int c = q; c < n; c += lpr) { const float d = row[c] - mean; d2 = fmaf(d, d, d2); }
        for (int o = 1; o < lpr; o <<= 1) d2 += __shfl_xor(d2, o);
        const float rstd = 1.0f / sqrtf(d2 * inv_n + 1e-5f);
        const float* const g = a.gamma;
        const float* const be = a.beta;
        for (int c = q; c < n; c += lpr) row[c] = (row[c] - mean) * rstd * g[c] + be[c];
    }
}

template <int ACT>
__global__ __launch_bounds__(CSP_BLOCK) void cspfit_bwd_row_kernel(CspfitRowArgs a) {
    const int t = threadIdx.x, lpr = a.lpr, rpw = CSP_BLOCK / lpr, q = t % lpr, n = a.n;
    const int64_t groups = ((int64_t)a.R + rpw - 1) / rpw;
    for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int64_t r = grp * rpw + t / lpr;
        if (r >= a.R) continue;                             // (the lpr lanes of a row leave together)
        const float* const zr = a.z + r * n;
        const float* const dyr = a.dy + r * n;
        const float* const xr = a.xin ? a.xin + r * n : nullptr;
        float* const dzr = a.dz + r * n;
        float* const dsr = a.ds ? a.ds + r * n : nullptr;
        float mean = 0.0f, rstd = 1.0f, m1 = 0.0f, m2 = 0.0f;
        if (a.gamma) {
            // the forward's S and statistics again, in its order; S, then xhat, staged in the row of dZ
            float* const dyxr = a.dyx + r * n;
            float s = 0.0f;
            for (int c = q; c < n; c += lpr) {
                float v = csp_activation<ACT>(zr[c]);
                if (a.drop_on) v *= cspfit_drop(a.drop_key, a.drop_thresh, a.drop_scale, (uint32_t)r, (uint32_t)c);
                if (xr) v += xr[c];
                dzr[c] = v;
                s += v;
            }
            const float inv_n = 1.0f / (float)n;
            for (int o = 1; o < lpr; o <<= 1) s += __shfl_xor(s, o);
            mean = s * inv_n;
            float d2 = 0.0f;
            for (int c = q; c < n; c += lpr) { const float d = dzr[c] - mean; d2 = fmaf(d, d, d2); }
            for (int o = 1; o < lpr; o <<= 1) d2 += __shfl_xor(d2, o);
            rstd = 1.0f / sqrtf(d2 * inv_n + 1e-5f);
            float s1 = 0.0f, s2 = 0.0f;
            for (int c = q; c < n; c += lpr) {
                const float xh = (dzr[c] - mean) * rstd;
                const float gdy = a.gamma[c] * dyr[c];
                s1 += gdy;
                s2 = fmaf(gdy, xh, s2);
                dyxr[c] = dyr[c] * xh;
                dzr[c] = xh;
            }
            for (int o = 1; o < lpr; o <<= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
            m1 = s1 * inv_n;
            m2 = s2 * inv_n;
        }
        for (int c = q; c < n; c += lpr) {
            const float z = zr[c];
            float ds = dyr[c];
            if (a.gamma) ds = rstd * ((a.gamma[c] * ds - m1) - dzr[c] * m2);
            float dz = ds * cspfit_act_prime<ACT>(z);
            if (a.drop_on) dz *= cspfit_drop(a.drop_key, a.drop_thresh, a.drop_scale, (uint32_t)r, (uint32_t)c);
            if (dsr) dsr[c] = ds;
            dzr[c] = dz;
        }
    }
}

struct CspfitColsumArgs {
    const float* src0; const float* src1; const float* src2;   // (R, n) each: dZ, dY * xhat, dY
    float* p0; float* p1; float* p2;     // ADAM: the vectors b, gamma, beta, and at the same offset from m / v their moments
    float* out0; float* out1; float* out2;   // gradient only: db, dgamma, dbeta
    int64_t m_delta, v_delta;            // floats from a parameter to its first / second moment
    int32_t R, n, kinds;
    HeadfitUpdateArgs adam;              // (the scalars of Adam alone)
};

template <bool ADAM>
__global__ __launch_bounds__(range_host::CSPFIT_COLSUM_BLOCK) void cspfit_colsum_kernel(CspfitColsumArgs a) {
    constexpr int U = 32;
    const int total = a.kinds * a.n;
    for (int idx = blockIdx.x * range_host::CSPFIT_COLSUM_BLOCK + threadIdx.x; idx < total;
         idx += gridDim.x * range_host::CSPFIT_COLSUM_BLOCK) {
        const int kind = idx / a.n, c = idx - kind * a.n;
        const float* const src = (kind == 0 ? a.src0 : kind == 1 ? a.src1 : a.src2) + c;
        float s = 0.0f;
        for (int r0 = 0; r0 < a.R; r0 += U) {
            float v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = r0 + u < a.R ? src[(int64_t)(r0 + u) * a.n] : 0.0f;
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (r0 + u < a.R) s += v[u];
        }
        if (ADAM) {
            float* const p = (kind == 0 ? a.p0 : kind == 1 ? a.p1 : a.p2) + c;
            float w = p[0], m = p[a.m_delta], v = p[a.v_delta];
            headfit_adam(a.adam, s, w, m, v);
            p[0] = w; p[a.m_delta] = m; p[a.v_delta] = v;
        } else {
            (kind == 0 ? a.out0 : kind == 1 ? a.out1 : a.out2)[c] = s;
        }
    }
}

struct CspfitBackArgs {
    const float* a;          // (R, lda): dZ, or a panel of G
    const float* w;          // the packed weight (csp_pack_head) whose rows c0 .. c0 + kc - 1 are the k of this launch
    const float* addend;     // (R, N) added behind the chain (the skip's dS), or null
    float* out;              // (R, N)
    int64_t n_items;
    int32_t R, lda, kc, c0, k_groups, N, col_groups, first;   // first = 0: the chain continues from `out`
};

// out (+)= A W: item = (32-row tile, group of 128 columns), a wave one 32 x 32 tile; k in order, two a step
__global__ __launch_bounds__(CSP_BLOCK) void cspfit_back_kernel(CspfitBackArgs a) {
    constexpr int U = 8;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l31 = lane & 31, lh = lane >> 5;
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const int64_t rt = item / a.col_groups;
        const int cg = (int)(item - rt * a.col_groups);
        const int col0 = (cg * 4 + wave) * 32;
        if (col0 >= a.N) continue;
        const int64_t arow = rt * 32 + l31;
        const bool arow_live = arow < a.R;
        const int col = col0 + l31;
        const bool col_live = col < a.N;
        // W[c][col] in the packed layout: ((c >> 5) k_groups + (col >> 3)) * 64 + 32 (col & 1) + (c & 31) float4s, component (col & 7) >> 1
        const size_t wcol = ((size_t)(col >> 3) * 64 + 32 * (col & 1)) * 4 + ((col & 7) >> 1);
        csp_f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t orow = rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            acc[r] = !a.first && col_live && orow < a.R ? a.out[orow * a.N + col] : 0.0f;
        }
        for (int k0 = 0; k0 < a.kc; k0 += 2 * U) {
            float av[U], bv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = k0 + 2 * u + lh;
                const bool live = k < a.kc;
                const int c = a.c0 + k;
                av[u] = live && arow_live ? a.a[arow * a.lda + k] : 0.0f;
                bv[u] = live && col_live ? a.w[((size_t)(c >> 5) * a.k_groups * 64 + (c & 31)) * 4 + wcol] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (k0 + 2 * u < a.kc) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
        }
        // element r of a lane: row (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column lane & 31 of the tile
        if (!col_live) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t orow = rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (orow < a.R) {
                float v = acc[r];
                if (a.addend) v += a.addend[orow * a.N + col];
                a.out[orow * a.N + col] = v;
            }
        }
    }
}

}  // namespace range_hip
