// The nearest support point of every query by haversine distance - the reference's assign_closest_label and
// the nearest-neighbour statistic of calc_avg_distances (evaluation/checkerboarddataset.py:78-107, :175-194),
// which build the whole (support x samples) float64 matrix there - as one scan that stores nothing per pair.
//
// THE TERM.  For query i and support j, in float64 and in the reference's expression order
//     dlon = lon2[j] - lon1[i];  dlat = lat2[j] - lat1[i]                                    (radians)
//     a    = sin(dlat/2) * sin(dlat/2) + (cos(lat1[i]) * cos(lat2[j])) * (sin(dlon/2) * sin(dlon/2))
// every sum and product a rounded one (checker_term is compiled with contraction off; the toolchain's
// __dadd_rn / __dmul_rn are plain operators that may still be fused), so `a` is numpy's up to the device's
// sin / cos.  The reference's distance c = 2 atan2(sqrt(a), sqrt(1 - a)) grows with a: the scan selects on a
// and maps the winner to c ONCE per query.  Ties go to the lower index (numpy.argmin); a pair whose a is NaN
// never wins (`a < best` is false); a query without a valid pair gets index -1 and distance NaN.
//
// WORK SPLIT.  One thread per query: lon1, lat1, cos(lat1) and the running (a, index) stay in registers.  A
// workgroup of 256 queries walks support tiles of CHECKER_TILE points: the 256 threads load one point each,
// form cos(lat2) ONCE for it, and put (lon, lat, cos lat) into LDS; in the pair loop every lane reads the same
// LDS address - a broadcast, no bank conflicts.  blockIdx.y is the chunk: it walks the tiles y, y + gridDim.y,
// ... (ascending j within a thread, so `<` alone keeps the lowest index of a chunk); blockIdx.x walks the
// query blocks grid-stride.  Every index is 64-bit.  With one chunk the result is written by the scan itself;
// with more, chunk y writes (a, index) of query i to part_a / part_idx[y * Q + i] and checker_merge_kernel
// picks the smaller a, then the smaller index, and maps a to c.  A pair's a does not depend on the split and
// the order (a, index) is total, so neither does the result.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_plan.h"

namespace range_hip {

using range_host::CHECKER_BLOCK;
using range_host::CHECKER_TILE;

struct CheckerArgs {
    const double* q;        // (Q,2) float64 (lon, lat) radians
    const double* s;        // (S,2) float64 (lon, lat) radians
    int64_t Q, S;
    int64_t q_blocks;       // ceil(Q / CHECKER_BLOCK)
    int64_t s_tiles;        // ceil(S / CHECKER_TILE)
    int32_t exclude_self;   // skip the pair j == i
    double* part_a;         // gridDim.y > 1: (chunks, Q) partial minima ...
    int64_t* part_idx;      // ... and their indices
    int64_t* idx;           // (Q)
    double* dist;           // (Q) or null
};

// a of one pair: (lon1, lat1, c1 = cos lat1) the query, (lon2, lat2, c2 = cos lat2) the support point
__device__ __forceinline__ double checker_term(double lon1, double lat1, double c1, double lon2, double lat2, double c2) {
#pragma clang fp contract(off)
    const double dlon = lon2 - lon1;
    const double dlat = lat2 - lat1;
    const double sh = sin(dlat * 0.5);       // dlat / 2, exactly
    const double sl = sin(dlon * 0.5);
    const double hh = sh * sh;
    const double cc = c1 * c2;
    const double ll = sl * sl;
    const double cl = cc * ll;
    return hh + cl;
}

// the reference's c at radius 1 for the winning a (checkerboarddataset.py:97); no winner: NaN
__device__ __forceinline__ double checker_distance(double a, int64_t idx) {
#pragma clang fp contract(off)
    if (idx < 0) return __builtin_nan("");
    const double r = 1.0 - a;
    return 2.0 * atan2(sqrt(a), sqrt(r));
}

__global__ __launch_bounds__(CHECKER_BLOCK) void checker_scan_kernel(CheckerArgs p) {
    extern __shared__ __attribute__((aligned(16))) double ck_lds[];
    double* const s_lon = ck_lds;
    double* const s_lat = ck_lds + CHECKER_TILE;
    double* const s_cos = ck_lds + 2 * CHECKER_TILE;
    const int t = threadIdx.x;
    for (int64_t qb = blockIdx.x; qb < p.q_blocks; qb += gridDim.x) {
        const int64_t i = qb * CHECKER_BLOCK + t;
        const bool live = i < p.Q;
        double lon1 = 0.0, lat1 = 0.0, c1 = 0.0;
        if (live) {
            lon1 = p.q[2 * i];
            lat1 = p.q[2 * i + 1];
            c1 = cos(lat1);
        }
        double best = __builtin_inf();
        int64_t best_j = -1;
        for (int64_t tile = blockIdx.y; tile < p.s_tiles; tile += gridDim.y) {
            const int64_t j0 = tile * CHECKER_TILE;
            const int n = (int)(p.S - j0 < CHECKER_TILE ? p.S - j0 : CHECKER_TILE);   // block-uniform
            __syncthreads();                                   // the previous tile has been read
            for (int k = t; k < n; k += CHECKER_BLOCK) {
                const double lon2 = p.s[2 * (j0 + k)], lat2 = p.s[2 * (j0 + k) + 1];
                s_lon[k] = lon2;
                s_lat[k] = lat2;
                s_cos[k] = cos(lat2);
            }
            __syncthreads();
            if (live) {
                const int skip = p.exclude_self && i >= j0 && i < j0 + n ? (int)(i - j0) : -1;
                for (int k = 0; k < n; ++k) {
                    const double a = checker_term(lon1, lat1, c1, s_lon[k], s_lat[k], s_cos[k]);
                    if (a < best && k != skip) {
                        best = a;
                        best_j = j0 + k;
                    }
                }
            }
        }
        if (live) {
            if (gridDim.y == 1) {
                p.idx[i] = best_j;
                if (p.dist) p.dist[i] = checker_distance(best, best_j);
            } else {
                p.part_a[(int64_t)blockIdx.y * p.Q + i] = best;
                p.part_idx[(int64_t)blockIdx.y * p.Q + i] = best_j;
            }
        }
    }
}

// the chunks' (a, index) of a query -> the smaller a, then the smaller index; chunks without a valid pair (-1) never win
__global__ __launch_bounds__(CHECKER_BLOCK) void checker_merge_kernel(const double* part_a, const int64_t* part_idx, int32_t chunks,
                                                                      int64_t Q, int64_t* idx, double* dist) {
    for (int64_t i = (int64_t)blockIdx.x * CHECKER_BLOCK + threadIdx.x; i < Q; i += (int64_t)gridDim.x * CHECKER_BLOCK) {
        double best = __builtin_inf();
        int64_t best_j = -1;
        for (int c = 0; c < chunks; ++c) {
            const double a = part_a[(int64_t)c * Q + i];
            const int64_t j = part_idx[(int64_t)c * Q + i];
            if (j >= 0 && (best_j < 0 || a < best || (a == best && j < best_j))) {
                best = a;
                best_j = j;
            }
        }
        idx[i] = best_j;
        if (dist) dist[i] = checker_distance(best, best_j);
    }
}

}  // namespace range_hip
