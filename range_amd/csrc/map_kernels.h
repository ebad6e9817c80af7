// Device side of the embedding map (include/range_map.h; reference: range/evaluation/
// visualize_embeddings.py:120-139, i.e. scikit-learn's FastICA with the logcosh contrast and
// skimage.exposure.equalize_hist).  All arithmetic is float64.  The pieces:
//   * map_project_kernel: the skinny projection Y = K (X - mean)^T, HBM-bound, X read once with 16-byte
//     loads, every row's c dot products from that one read;
//   * map_ica_step_kernel + map_fold_kernel: the two reductions of a parallel-FastICA step in one fixed
//     order (thread, wave, workgroup through LDS, one slab per row chunk, slabs in index order) - no
//     floating-point atomics;
//   * map_sources_kernel: S = (M Y)^T;
//   * map_hist_kernel + map_equalize_kernel: numpy.histogram's uniform-bin rule with integer counts (LDS
//     histograms, then integer atomics), the normalised cumulative sum and numpy.interp at the bin centres.
// The launch geometry is range_host::map_plan (host_plan.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_plan.h"

namespace range_map {

using range_host::MAP_BLOCK;
using range_host::MAP_MAX_BINS;
using range_host::MAP_PROJ_ROWS;
using range_host::MAP_PROJ_WAVE_ROWS;

constexpr int MAP_WAVES = MAP_BLOCK / 64;

struct MapMat {
    double m[64];   // c x c, row-major, c <= 8
};

// ------------------------------------------------------------------------------------------
// Y[k, i] = sum_j K[k, j] * (X[i, j] - mean[j]).  A wave takes MAP_PROJ_WAVE_ROWS rows a trip; lane l owns
// the column pairs 2l, 2l + 128, ...: per pair it loads K and the mean once and one 16-byte piece of each of
// its rows, so K costs c/8 of the traffic of X.  The R * C partial dot products are summed over the lanes by
// a butterfly and stored through LDS, component-major.  VEC: X is 16-byte aligned and ldx is even.
template <int C, bool VEC>
__global__ __launch_bounds__(MAP_BLOCK) void map_project_kernel(const double* __restrict__ X, int64_t n,
                                                                int32_t d, int64_t ldx,
                                                                const double* __restrict__ mean,
                                                                const double* __restrict__ K,
                                                                double* __restrict__ Y, int64_t ldy,
                                                                int64_t groups) {
    constexpr int R = MAP_PROJ_WAVE_ROWS;
    __shared__ double sh[MAP_WAVES][C * R];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t row0 = g * MAP_PROJ_ROWS + (int64_t)w * R;
        double acc[R][C];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int k = 0; k < C; ++k) acc[r][k] = 0.0;
        for (int col = 2 * lane; col < d; col += 128) {
            const bool two = col + 1 < d;
            const double m0 = mean ? mean[col] : 0.0;
            const double m1 = (mean && two) ? mean[col + 1] : 0.0;
            double k0[C], k1[C];
#pragma unroll
            for (int k = 0; k < C; ++k) {
                k0[k] = K[(int64_t)k * d + col];
                k1[k] = two ? K[(int64_t)k * d + col + 1] : 0.0;
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int64_t row = row0 + r;
                if (row >= n) continue;          // the same in every lane of the wave
                const double* p = X + row * ldx + col;
                double x0, x1;
                if (VEC && two) {
                    const double2 v = *reinterpret_cast<const double2*>(p);
                    x0 = v.x;
                    x1 = v.y;
                } else {
                    x0 = p[0];
                    x1 = two ? p[1] : 0.0;
                }
                x0 -= m0;
                x1 -= m1;
#pragma unroll
                for (int k = 0; k < C; ++k) acc[r][k] = fma(k1[k], x1, fma(k0[k], x0, acc[r][k]));
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int k = 0; k < C; ++k) {
                double v = acc[r][k];
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
                if (lane == 0) sh[w][k * R + r] = v;
            }
        __syncthreads();
        if (lane < C * R) {
            const int k = lane / R, r = lane % R;
            const int64_t row = row0 + r;
            if (row < n) Y[(int64_t)k * ldy + row] = sh[w][lane];
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// w . y to (nearly) the last bit: products split exactly by fma, sums by TwoSum, so that the argument of tanh
// carries one rounding however much the c products cancel.
template <int C>
__device__ inline double map_dot(const double* __restrict__ w, const double (&y)[C]) {
#pragma clang fp contract(off)
    double hi = 0.0, lo = 0.0;
#pragma unroll
    for (int l = 0; l < C; ++l) {
        const double p = w[l] * y[l];
        const double pe = fma(w[l], y[l], -p);
        const double s = hi + p;
        const double bb = s - hi;
        const double se = (hi - (s - bb)) + (p - bb);
        hi = s;
        lo += pe + se;
    }
    return hi + lo;
}

// 1 - tanh^2(u) = 4 e / (1 + e)^2 with e = exp(-2|u|): a few ulps of the value at every u, where 1 - t*t
// loses as many digits as t has nines.
__device__ inline double map_sech2(double u) {
    const double e = exp(-2.0 * fabs(u));
    const double q = 1.0 + e;
    return 4.0 * e / (q * q);
}

// One parallel-FastICA step's sums over the rows of slab s = rows [s * ipt * 256, (s + 1) * ipt * 256):
// slab[s][k*C + l] = sum tanh(w_k . y_i) Y[l, i], slab[s][C*C + k] = sum (1 - tanh^2(w_k . y_i)).
// Order: a thread adds its ipt rows in index order, a wave its lanes by the shfl_down tree, the workgroup its
// four waves in wave order.  Which workgroup computes a slab does not matter.
template <int C>
__global__ __launch_bounds__(MAP_BLOCK) void map_ica_step_kernel(const double* __restrict__ Y, int64_t n,
                                                                 int64_t ldy, MapMat W, int64_t ipt,
                                                                 int64_t slabs,
                                                                 double* __restrict__ slab_out) {
    constexpr int V = C * C + C;
    __shared__ double sh[MAP_WAVES][V];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int64_t s = blockIdx.x; s < slabs; s += gridDim.x) {
        double acc[V];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = 0.0;
        const int64_t base = s * ipt * MAP_BLOCK + threadIdx.x;
        for (int64_t j = 0; j < ipt; ++j) {
            const int64_t i = base + j * MAP_BLOCK;
            if (i >= n) break;
            double y[C];
#pragma unroll
            for (int l = 0; l < C; ++l) y[l] = Y[(int64_t)l * ldy + i];
#pragma unroll
            for (int k = 0; k < C; ++k) {
                const double u = map_dot<C>(W.m + k * C, y);
                const double t = tanh(u);
#pragma unroll
                for (int l = 0; l < C; ++l) acc[k * C + l] = fma(t, y[l], acc[k * C + l]);
                acc[C * C + k] += map_sech2(u);
            }
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            double x = acc[v];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) x += __shfl_down(x, off, 64);
            if (lane == 0) sh[w][v] = x;
        }
        __syncthreads();
        if (threadIdx.x < V) {
            double x = sh[0][threadIdx.x];
#pragma unroll
            for (int i = 1; i < MAP_WAVES; ++i) x += sh[i][threadIdx.x];
            slab_out[s * V + threadIdx.x] = x;
        }
        __syncthreads();
    }
}

// out[v] = slab[0][v] + slab[1][v] + ... in index order.  One workgroup: the slabs pass through LDS a tile at a
// time (all threads load, coalesced), thread v adds its column of the tile in slab order - the serial chain is the
// additions, not the loads.
constexpr int MAP_FOLD_DOUBLES = 4096;
__global__ __launch_bounds__(MAP_BLOCK) void map_fold_kernel(const double* __restrict__ slab, int64_t slabs,
                                                             int32_t V, double* __restrict__ out) {
    __shared__ double sh[MAP_FOLD_DOUBLES];
    const int tile = MAP_FOLD_DOUBLES / V;          // slabs a tile; V <= 72
    const int v = threadIdx.x;
    double x = 0.0;
    for (int64_t s0 = 0; s0 < slabs; s0 += tile) {
        const int cnt = (int)(slabs - s0 < tile ? slabs - s0 : tile);
        for (int e = threadIdx.x; e < cnt * V; e += MAP_BLOCK) sh[e] = slab[s0 * V + e];
        __syncthreads();
        if (v < V)
            for (int s = 0; s < cnt; ++s) x += sh[s * V + v];
        __syncthreads();
    }
    if (v < V) out[v] = x;
}

// S[i, k] = sum_l M[k, l] * Y[l, i]
template <int C>
__global__ __launch_bounds__(MAP_BLOCK) void map_sources_kernel(const double* __restrict__ Y, int64_t n,
                                                                int64_t ldy, MapMat M,
                                                                double* __restrict__ S) {
    for (int64_t i = (int64_t)blockIdx.x * MAP_BLOCK + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * MAP_BLOCK) {
        double y[C];
#pragma unroll
        for (int l = 0; l < C; ++l) y[l] = Y[(int64_t)l * ldy + i];
#pragma unroll
        for (int k = 0; k < C; ++k) {
            double v = 0.0;
#pragma unroll
            for (int l = 0; l < C; ++l) v = fma(M.m[k * C + l], y[l], v);
            S[i * C + k] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------
// numpy.histogram's rule for uniform bins (numpy/lib/_histograms_impl.py): the index is
// trunc((x - first) / (last - first) * nbins), nbins -> nbins - 1, one down when x < edges[index], one up when
// x >= edges[index + 1] unless it is the last bin.  x is in [first, last].
__device__ inline int map_bin(double x, const double* e, int nbins, double first, double denom) {
#pragma clang fp contract(off)
    const double f = ((x - first) / denom) * (double)nbins;
    int idx = (int)f;
    if (idx >= nbins) idx = nbins - 1;
    if (idx < 0) idx = 0;
    if (x < e[idx] && idx > 0) --idx;
    if (idx != nbins - 1 && x >= e[idx + 1]) ++idx;
    return idx;
}

__global__ __launch_bounds__(MAP_BLOCK) void map_hist_kernel(const double* __restrict__ x, int64_t n,
                                                             int64_t ldx,
                                                             const double* __restrict__ edges,
                                                             int32_t nbins,
                                                             unsigned long long* __restrict__ counts) {
    __shared__ double e[MAP_MAX_BINS + 1];
    __shared__ unsigned int h[MAP_MAX_BINS];
    for (int b = threadIdx.x; b <= nbins; b += MAP_BLOCK) e[b] = edges[b];
    for (int b = threadIdx.x; b < nbins; b += MAP_BLOCK) h[b] = 0u;
    __syncthreads();
    const double first = e[0], last = e[nbins], denom = last - first;
    for (int64_t i = (int64_t)blockIdx.x * MAP_BLOCK + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * MAP_BLOCK) {
        const double v = x[i * ldx];
        if (v >= first && v <= last) atomicAdd(&h[map_bin(v, e, nbins, first, denom)], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < nbins; b += MAP_BLOCK)
        if (h[b]) atomicAdd(&counts[b], (unsigned long long)h[b]);
}

// out = numpy.interp(x, centres, cdf): cdf[b] = (counts[0] + ... + counts[b]) / total as float64,
// centres[b] = (edges[b] + edges[b + 1]) / 2; below the first centre cdf[0], above the last cdf[nbins - 1],
// on a centre its cdf, between two centres slope * (x - centre[j]) + cdf[j] (numpy's arr_interp).
// skimage.exposure.equalize_hist of a float image with nbins bins is exactly this on its own histogram.
// Every workgroup rebuilds the nbins centres and cdf values in its LDS from the counts (a few KB from L2): no table
// in device memory that two streams would share.  Conditions the caller keeps: the edges increase strictly (the
// last centre <= x is taken from x's bin, b or b - 1; a range of a few ulps, where numpy.linspace repeats edges,
// is not covered and may differ from numpy.interp's search); when no value lies in [first, last] the total is 0
// and every output is NaN.
__global__ __launch_bounds__(MAP_BLOCK) void map_equalize_kernel(const double* __restrict__ x, int64_t n,
                                                                 int64_t ldx,
                                                                 const double* __restrict__ edges,
                                                                 int32_t nbins,
                                                                 const unsigned long long* __restrict__ counts,
                                                                 double* __restrict__ out, int64_t ldo) {
#pragma clang fp contract(off)
    __shared__ double e[MAP_MAX_BINS + 1];
    __shared__ double ctr[MAP_MAX_BINS];
    __shared__ double cdf[MAP_MAX_BINS];
    __shared__ unsigned long long cum[MAP_MAX_BINS];
    for (int b = threadIdx.x; b <= nbins; b += MAP_BLOCK) e[b] = edges[b];
    for (int b = threadIdx.x; b < nbins; b += MAP_BLOCK) cum[b] = counts[b];
    __syncthreads();
    if (threadIdx.x == 0) {                         // the running sum over LDS: no load waits on another
        unsigned long long run = 0;
        for (int b = 0; b < nbins; ++b) {
            run += cum[b];
            cum[b] = run;
        }
    }
    __syncthreads();
    const double total = (double)cum[nbins - 1];
    for (int b = threadIdx.x; b < nbins; b += MAP_BLOCK) {
        ctr[b] = (e[b] + e[b + 1]) / 2.0;
        cdf[b] = (double)cum[b] / total;
    }
    __syncthreads();
    const double first = e[0], denom = e[nbins] - e[0];
    for (int64_t i = (int64_t)blockIdx.x * MAP_BLOCK + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * MAP_BLOCK) {
        const double v = x[i * ldx];
        double r;
        if (v != v) r = v;
        else if (v < ctr[0]) r = cdf[0];
        else if (v > ctr[nbins - 1]) r = cdf[nbins - 1];
        else {
            const int b = map_bin(v, e, nbins, first, denom);
            int j = (v >= ctr[b]) ? b : b - 1;           // the last centre <= v (b >= 1 when v < ctr[b])
            if (j < 0) j = 0;
            if (j >= nbins - 1) r = cdf[nbins - 1];
            else if (ctr[j] == v) r = cdf[j];
            else {
                const double slope = (cdf[j + 1] - cdf[j]) / (ctr[j + 1] - ctr[j]);
                r = slope * (v - ctr[j]) + cdf[j];
            }
        }
        out[i * ldo] = r;
    }
}

}  // namespace range_map
