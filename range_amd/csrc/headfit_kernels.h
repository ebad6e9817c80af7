// The fit of the CSP class head from frozen embeddings (include/range_headfit.h; host_plan.h: headfit_plan): one
// step of the reference's supervised stage (csp/main/losses.py:395-470 embedding_loss without 'user', under
// torch.optim.Adam) with the location encoder frozen, i.e. on the one matrix class_emb W (C, F).
//
//   z = x W^T, p = sigmoid(z);   loss = mean_{B x C}(Lpos) + weight * mean_{Bg x C}(Lbg)
//   Lbg = -log(1 - p + 1e-5);  Lpos the same, at the label's column -C log(p + 1e-5)
//   dL/dz: negatives p (1 - p) / (1 - p + 1e-5) / (B C)  [background rows: * weight / (Bg C)],
//          the label's column -C p (1 - p) / (p + 1e-5) / (B C);      dW = G^T [X; Xbg]
//
// ROWS.  headfit_gather_kernel writes the step's rows - B rows of the (N, F) feature matrix picked by an int32
// id array (clamped to 0 .. N - 1; without ids rows 0 .. B - 1), then the Bg background rows - as one (R, F)
// matrix X: both products read it.
//
// LOGIT GRADIENT (headfit_grad_kernel).  The head's tile and chain (csp_head_kernel.h: csp_head_load_x,
// csp_head_gemm on v_mfma_f32_32x32x2_f32) over the current W in the packed layout of csp_pack_head.  An item is
// a row tile with one chunk of the panel's class tiles.  The epilogue forms p with the head's sigmoid, stores
// G (R, panel_cols) and, per 32-class tile and row, the sum of the negative terms (the 32 lanes folded by a
// fixed xor tree) and the label term -log(p + 1e-5) (at most one lane holds it): a tile's sums depend on the
// row and the tile alone.  headfit_fold_kernel adds a panel's tiles to the running row sums in tile order, so the
// sums are ONE tile-ordered chain whatever the panel width.  A label outside 0 .. C - 1 matches no column.
//
// UPDATE (headfit_update_kernel).  dW^T tile = X^T G on the same MFMA: A[m = feature][k = row] from X, B[k = row]
// [n = class] straight from G (for a fixed row 32 lanes read 32 consecutive classes), every output ONE chain
// ordered by row index over the R rows.  A wave holds two 32-feature tiles of one class tile; a lane's results
// are then one class and features (r & 3) + 8 (r >> 2) + 4 (lane >> 5): in the packed layout pairs of them are
// 8 adjacent bytes and the 64 lanes cover 512 contiguous bytes, so Adam - elementwise, W, m and v all in that
// layout - reads and writes whole lines in place.  Without Adam the tile is stored unpacked as dW (C, F).
//
// No atomics.  Classes are independent given X, so neither the panel width nor the grid changes a bit of G, dW,
// W or the row sums.  headfit_loss_kernel (one workgroup) folds the row sums to three scalars in a fixed order.
// A NaN feature row gives NaN logits, hence NaN in its row of G and in dW, as in torch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csp_head_kernel.h"
#include "host_plan.h"

namespace range_hip {

constexpr float HEADFIT_LOG_EPS = 1e-5f;        // losses.py: the 1e-5 inside both logarithms

__global__ __launch_bounds__(CSP_BLOCK) void headfit_gather_kernel(const float* feats, int64_t N, const int32_t* rows,
                                                                   int32_t B, const float* bg, int32_t R, int32_t K, float* x) {
    const int64_t total = (int64_t)R * K;
    for (int64_t i = (int64_t)blockIdx.x * CSP_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * CSP_BLOCK) {
        const int32_t r = (int32_t)(i / K), k = (int32_t)(i - (int64_t)r * K);
        float v;
        if (r < B) {
            int64_t id = rows ? (int64_t)rows[r] : (int64_t)r;
            id = id < 0 ? 0 : id < N ? id : N - 1;
            v = feats[id * K + k];
        } else {
            v = bg[(int64_t)(r - B) * K + k];
        }
        x[i] = v;
    }
}

struct HeadfitGradArgs {
    const float* x;          // (R, K) gathered rows
    const float4* w4;        // packed W
    const int32_t* labels;   // (B)
    float* g;                // (R, panel_cols); unused without WRITE_G
    float* parts;            // (2, panel_tiles, R): negative sums, label terms
    int64_t n_items;
    int32_t R, B, K, k_groups, ld, C, tile0, n_tiles, n_chunks, panel_tiles, panel_cols;
    float s_neg, s_lab, s_bg;   // 1 / (B C), -C / (B C), weight / (Bg C)
};

template <int MT, bool WRITE_G>
__global__ __launch_bounds__(CSP_BLOCK, 2) void headfit_grad_kernel(HeadfitGradArgs a) {
    constexpr int T = 32 * MT;
    constexpr int NT = CSP_HEAD_ACC_TILES / MT;
    extern __shared__ __attribute__((aligned(16))) float hf_x[];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l31 = lane & 31, lh = lane >> 5;
    const int ld = a.ld, K = a.K, k_pad = a.k_groups * 8;
    int32_t* const lab = reinterpret_cast<int32_t*>(hf_x + T * ld);     // the tile's labels; -1: a background row
    const bool vec4 = K % 4 == 0 && reinterpret_cast<uintptr_t>(a.x) % 16 == 0;
    int64_t loaded = -1;
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const int64_t rt = item / a.n_chunks;
        const int ch = (int)(item - rt * a.n_chunks);
        const int b0 = (int)rt * T;
        if (rt != loaded) {
            __syncthreads();
            csp_head_load_x<T>(a.x, a.R, b0, K, k_pad, ld, vec4, hf_x, wave, lane);
            if (t < T) lab[t] = b0 + t < a.B ? a.labels[b0 + t] : -1;
            __syncthreads();
            loaded = rt;
        }
        const int t0 = ch * 4 * NT + wave;       // this wave's tiles of the panel: t0, t0 + 4, ...
        int ntw = a.n_tiles > t0 ? (a.n_tiles - t0 + 3) / 4 : 0;
        ntw = ntw < NT ? ntw : NT;
        if (ntw == 0) continue;
        uint32_t base[NT];
        int col[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int c = (a.tile0 + t0 + 4 * j) * 32 + l31;
            const int cc = c < a.C ? c : a.C - 1;
            col[j] = c;
            base[j] = ((uint32_t)(cc >> 5) * (uint32_t)a.k_groups) * 64u + 32u * lh + (uint32_t)(cc & 31);
        }
        csp_f32x16 acc[MT][NT];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][j][r] = 0.0f;
        csp_head_gemm_dispatch<MT, NT>(acc, ntw, a.w4, base, a.k_groups, hf_x + l31 * ld + lh, 32 * ld);
        // element r of a lane is row (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column lane & 31 of its 32x32 tile
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            if (j < ntw) {
                const int lt = t0 + 4 * j;
                const bool col_live = col[j] < a.C;
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int rl = m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                        const int row = b0 + rl;
                        const bool row_live = row < a.R;
                        const bool is_lab = col_live && row_live && col[j] == lab[rl];
                        const float p = csp_activation<range_host::CSP_ACT_SIGMOID>(acc[m][j][r]);
                        const float q = 1.0f - p;
                        const float den = (is_lab ? p : q) + HEADFIT_LOG_EPS;
                        const float term = -logf(den);
                        if (WRITE_G) {
                            const float s = is_lab ? a.s_lab : row < a.B ? a.s_neg : a.s_bg;
                            if (col_live && row_live) a.g[(int64_t)row * a.panel_cols + (lt * 32 + l31)] = s * (p * q / den);
                        }
                        float neg = col_live && !is_lab ? term : 0.0f;
#pragma unroll
                        for (int o = 1; o < 32; o <<= 1) neg += __shfl_xor(neg, o);
                        // the label term: the one lane of the 32 that holds it writes it, else lane 0 writes 0
                        const unsigned long long hit = __ballot(is_lab);
                        const bool any = ((hit >> (32 * lh)) & 0xffffffffull) != 0;
                        if (row_live) {
                            if (l31 == 0) a.parts[(int64_t)lt * a.R + row] = neg;
                            if (any ? is_lab : l31 == 0) a.parts[((int64_t)a.panel_tiles + lt) * a.R + row] = is_lab ? term : 0.0f;
                        }
                    }
            }
        }
    }
}

// rowsum (2, R) += the panel's tiles, in tile order (first: the chain starts from 0)
__global__ __launch_bounds__(CSP_BLOCK) void headfit_fold_kernel(const float* parts, float* rowsum, int32_t R, int32_t n_tiles,
                                                                 int32_t panel_tiles, int32_t first) {
    for (int32_t row = blockIdx.x * CSP_BLOCK + threadIdx.x; row < R; row += gridDim.x * CSP_BLOCK)
        for (int kind = 0; kind < 2; ++kind) {
            float s = first ? 0.0f : rowsum[kind * R + row];
            for (int32_t lt = 0; lt < n_tiles; ++lt) s += parts[((int64_t)kind * panel_tiles + lt) * R + row];
            rowsum[kind * R + row] = s;
        }
}

// out[0] the loss, out[1] its batch part mean_{B x C}(Lpos), out[2] mean over the batch rows of -log(p_label + 1e-5)
// (trainer_helper.py: test()).  Thread t adds rows t, t + 256, ... in order; the 256 sums are folded by a fixed tree.
__global__ __launch_bounds__(CSP_BLOCK) void headfit_loss_kernel(const float* rowsum, int32_t R, int32_t B, int32_t C, float weight,
                                                                 float* out) {
    __shared__ float sh[3][CSP_BLOCK];
    const int t = threadIdx.x;
    float pos = 0.0f, lab = 0.0f, bg = 0.0f;
    for (int32_t row = t; row < R; row += CSP_BLOCK) {
        const float n = rowsum[row], l = rowsum[R + row];
        if (row < B) { pos += n + (float)C * l; lab += l; }
        else bg += n;
    }
    sh[0][t] = pos; sh[1][t] = lab; sh[2][t] = bg;
    __syncthreads();
    for (int o = CSP_BLOCK / 2; o > 0; o >>= 1) {
        if (t < o)
            for (int i = 0; i < 3; ++i) sh[i][t] += sh[i][t + o];
        __syncthreads();
    }
    if (t == 0) {
        const int32_t Bg = R - B;
        const float lpos = sh[0][0] / ((float)B * (float)C);
        const float lbg = Bg > 0 ? sh[2][0] / ((float)Bg * (float)C) : 0.0f;
        out[0] = lpos + weight * lbg;
        out[1] = lpos;
        out[2] = sh[1][0] / (float)B;
    }
}

struct HeadfitUpdateArgs {
    const float* x;          // (R, K)
    const float* g;          // (R, panel_cols)
    float* w; float* m; float* v;   // packed (csp_pack_head); ADAM only
    float* dw;               // (C, K); gradient only
    int64_t n_items;
    int32_t R, K, k_groups, C, tile0, panel_cols, f_groups;
    float wd, omb1, b2, omb2, eps, step_size, bc2_sqrt;
};

// torch.optim.Adam's single-tensor step on one element (no amsgrad): L2 weight decay into the gradient, the moments,
// denom = sqrt(v) / sqrt(1 - b2^t) + eps, w -= lr / (1 - b1^t) * m / denom
__device__ __forceinline__ void headfit_adam(const HeadfitUpdateArgs& a, float g, float& w, float& m, float& v) {
    if (a.wd != 0.0f) g += a.wd * w;
    m += (g - m) * a.omb1;
    v = v * a.b2 + a.omb2 * g * g;
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    w -= a.step_size * (m / denom);
}

template <bool ADAM>
__global__ __launch_bounds__(CSP_BLOCK) void headfit_update_kernel(HeadfitUpdateArgs a) {
    constexpr int U = 8;                     // row pairs whose operands are loaded ahead of their MFMAs
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l31 = lane & 31, lh = lane >> 5;
    const int K = a.K, R = a.R;
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const int lt = (int)(item / a.f_groups);
        const int fb = ((int)(item - (int64_t)lt * a.f_groups) * 4 + wave) * 64;     // this wave's 64 features
        if (fb >= K) continue;
        const bool two = fb + 32 < K;
        const int c = (a.tile0 + lt) * 32 + l31;
        const bool c_live = c < a.C;
        const int f0 = fb + l31, f1 = f0 + 32;
        const bool f0_live = f0 < K, f1_live = f1 < K;
        const float* const gp = a.g + (lt * 32 + l31);
        csp_f32x16 acc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
        for (int r0 = 0; r0 < R; r0 += 2 * U) {
            float bv[U], a0[U], a1[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int row = r0 + 2 * u + lh;
                const bool live = row < R;
                bv[u] = live && c_live ? gp[(int64_t)row * a.panel_cols] : 0.0f;
                a0[u] = live && f0_live ? a.x[(int64_t)row * K + f0] : 0.0f;
                a1[u] = live && f1_live ? a.x[(int64_t)row * K + f1] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (r0 + 2 * u < R) {
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[u], bv[u], acc[0], 0, 0, 0);
                    if (two) acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[u], bv[u], acc[1], 0, 0, 0);
                }
            }
        }
        // element r of a lane: feature fb + 32 j + (r & 3) + 8 (r >> 2) + 4 lh, class c
        if (!c_live) continue;
        if (ADAM) {
            const size_t tile = (size_t)(a.tile0 + lt) * a.k_groups;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int kg = fb / 8 + 4 * j + rr;
                    if (kg >= a.k_groups) continue;
#pragma unroll
                    for (int par = 0; par < 2; ++par) {
                        // features fa = 8 kg + 4 lh + par and fa + 2: components 2 lh, 2 lh + 1 of the class's fragment
                        const int fa = 8 * kg + 4 * lh + par;
                        const size_t at = ((tile + kg) * 64 + 32 * par + l31) * 4 + 2 * lh;
                        float2 w = *reinterpret_cast<float2*>(a.w + at);
                        float2 m = *reinterpret_cast<float2*>(a.m + at);
                        float2 v = *reinterpret_cast<float2*>(a.v + at);
                        if (fa < K) headfit_adam(a, acc[j][4 * rr + par], w.x, m.x, v.x);
                        if (fa + 2 < K) headfit_adam(a, acc[j][4 * rr + par + 2], w.y, m.y, v.y);
                        *reinterpret_cast<float2*>(a.w + at) = w;
                        *reinterpret_cast<float2*>(a.m + at) = m;
                        *reinterpret_cast<float2*>(a.v + at) = v;
                    }
                }
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int f = fb + 32 * j + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (f < K) a.dw[(int64_t)c * K + f] = acc[j][r];
                }
        }
    }
}

// the packed W as (C, K) row-major
__global__ __launch_bounds__(CSP_BLOCK) void headfit_unpack_kernel(const float* w, int32_t C, int32_t K, int32_t k_groups, float* out) {
    const int64_t total = (int64_t)C * K;
    for (int64_t i = (int64_t)blockIdx.x * CSP_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * CSP_BLOCK) {
        const int32_t n = (int32_t)(i / K), k = (int32_t)(i - (int64_t)n * K);
        const int kk = k & 7;
        out[i] = w[((((size_t)(n >> 5) * k_groups + (k >> 3)) * 64 + 32 * (kk & 1) + (n & 31)) * 4) + (kk >> 1)];
    }
}

}  // namespace range_hip
