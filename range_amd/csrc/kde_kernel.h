// The KDE geo prior of the CSP evaluation (location_models/csp/main/baselines.py: create_kde_grid, kde_prior), the
// sixth location-only baseline: a Gaussian kernel density over the binned training set with a per-query bandwidth.
// The reference queries a BallTree twice per sample and sums float weights per class in the tree's neighbour order.
// Here: the vote scan of neighbor_kernel.h with a WEIGHT per member, accumulated as 64-bit fixed-point integers so
// that, like the counts there, no result depends on the split, the grid, the stream, the order of the bins or on
// whether a bin of count n is installed as n bins of count 1.
//
// THE SET.  M bins (class, quantised location, count >= 1) are installed as NeighborPoints whose `cell` slot carries
// the count (range_set_kde_points); neighbor_select_kernel gives red_k of the kde_nb-th bin, unchanged.
//
// PER QUERY the host forms (range_amd/geo_baselines.py, in the reference's expressions) h = 0.5 d_k, r = 2 h + 1e-9,
//   thr    = what query_radius(r) compares red with (sin(r / 2)^2 or r^2); NaN: the query has no member
//   two_h2 = 2 h^2
// A bin j is a member when red(i, j) <= thr, red neighbor_red's.  Its weight, float64, nothing contracted:
//   dist = red                                                          (euclidean: dlat dlat + dlon dlon)
//   dist = (2 asin(sqrt(a)))^2, a = sin(dlat / 2)^2 + (cos lat_j cos lat_i) sin(dlon / 2)^2, d = bin - query
//                                                                       (haversine: utils.distance_pw_haversine's order)
//   w    = exp(-(dist / two_h2))                                        (a true division)
// and row[class_j] += count_j * (uint64) rint(w * 2^s) - one 64-bit LDS integer add.  s (host_plan.h:
// kde_scale_bits) is fixed at install time so that total_count * 2^s < 2^62: no row and no sum of rows overflows.
// dist <= (2 h)^2 up to the 1e-9, so w lies in [e^-2 - eps, 1]; a w that is no number in [0, 1] (two_h2 <= 0 or NaN:
// never from the host code above) counts as 0, or 1 above 1, so that the bound on the rows holds for any input.
//
// PRIOR.  (2 pi h)^-1 and kde_den cancel from the reference's result: with I_c the row, S = sum_c I_c (exact),
// m = min over I_c > 0:  prior[c] = ((double) I_c + (double) m) / ((double) S + (double) C * (double) m), and 1.0 / C
// when S == 0 (a NaN query).  Score, greater / tied_after / argmax and their flags: neighbor_rank_row.
//
// WORK SPLIT (host_plan.h: kde_plan): neighbor_vote_kernel's - G queries a workgroup (uint64 rows: half as many),
// 1024 threads, tiles of 256, NEIGHBOR_UNROLL trips of loads in flight, chunks over grid y; with more than one
// chunk the partial uint64 rows go to the workspace and kde_fold_kernel adds them and ranks.
#pragma once
#include "neighbor_kernel.h"

namespace range_hip {

struct KdeQuery {            // NEIGHBOR_QUERY_LDS bytes
    double lat, lon, cs;
    double thr, two_h2;
    double pad;
};
static_assert(sizeof(KdeQuery) == range_host::NEIGHBOR_QUERY_LDS, "layout");

struct KdeArgs {
    const NeighborPoint* pts;        // `cell` is the bin's count
    int64_t M, n_tiles;
    const double* q;                 // (B, 2) (lon, lat): radians (haversine) or degrees
    const double* thr;               // (B)
    const double* two_h2;            // (B)
    int64_t B, groups;
    int32_t G, C;
    double scale;                    // 2^s
    const void* img;                 // (B, C) float32 / float64 or null
    int32_t img_kind;
    const int32_t* labels;           // (B), with greater / tied / argmax
    int32_t *greater, *tied, *argmax;
    double* prior;                   // (B, C) or null
    uint64_t* sums;                  // (B, C) or null
    uint64_t* ws;                    // chunks > 1: (chunks, groups, G * C) partial rows
    int32_t chunks;                  // fold: how many
};

// the squared distance the reference weighs a member by
template <bool HAV>
__device__ __forceinline__ double kde_dist(const KdeQuery& q, const NeighborPoint& p, double red) {
#pragma clang fp contract(off)
    if (!HAV) return red;
    const double sa = sin((p.lat - q.lat) / 2.0);
    const double sb = sin((p.lon - q.lon) / 2.0);
    const double cos_term = p.cs * q.cs;
    const double a2 = sa * sa;
    const double b2 = sb * sb;
    const double cb = cos_term * b2;
    const double a = a2 + cb;
    const double d = 2.0 * asin(sqrt(a));
    return d * d;
}

__device__ __forceinline__ uint64_t kde_fixed(double dist, double two_h2, double scale) {
#pragma clang fp contract(off)
    const double arg = dist / two_h2;
    double w = exp(-arg);
    w = w <= 1.0 ? (w >= 0.0 ? w : 0.0) : (w != w ? 0.0 : 1.0);
    return (uint64_t)rint(w * scale);
}

// the rows of a group, a wave each: sums / priors on request, the three integers
__device__ __forceinline__ void kde_rank_group(const KdeArgs& a, const uint64_t* rows, int64_t b0, int live) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int C = a.C;
    for (int g = wave; g < live; g += NEIGHBOR_VOTE_BLOCK / 64) {
        const uint64_t* const row = rows + (size_t)g * C;
        const int64_t b = b0 + g;
        uint64_t sum = 0, mn = ~UINT64_C(0);
        for (int c = lane; c < C; c += 64) {
            const uint64_t v = row[c];
            sum += v;
            if (v != 0 && v < mn) mn = v;
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            sum += __shfl_xor(sum, o);
            const uint64_t om = __shfl_xor(mn, o);
            mn = om < mn ? om : mn;
        }
        const bool uniform = sum == 0;
        const double m = (double)mn, one_c = 1.0 / (double)C;
        const double den = (double)sum + (double)C * m;
        const auto prior_of = [&](uint64_t v) { return uniform ? one_c : ((double)v + m) / den; };
        if (a.sums)
            for (int c = lane; c < C; c += 64) a.sums[b * C + c] = row[c];
        if (a.prior)
            for (int c = lane; c < C; c += 64) a.prior[b * C + c] = prior_of(row[c]);
        if (!a.greater) continue;
        neighbor_rank_row(a.img, a.img_kind, a.labels, a.greater, a.tied, a.argmax, b, C, lane, [&](int c) { return prior_of(row[c]); });
    }
}

template <bool HAV>
__global__ __launch_bounds__(NEIGHBOR_VOTE_BLOCK) void kde_vote_kernel(KdeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t kde_lds[];
    const int t = threadIdx.x;
    const int G = a.G, C = a.C;
    const int row_words = G * C;                                  // at most NEIGHBOR_COUNT_LDS / 8
    uint64_t* const rows = kde_lds;
    KdeQuery* const qs = reinterpret_cast<KdeQuery*>(kde_lds + ((row_words + 1) & ~1));
    for (int64_t grp = blockIdx.x; grp < a.groups; grp += gridDim.x) {
        const int64_t b0 = grp * G;
        const int live = a.B - b0 < G ? (int)(a.B - b0) : G;
        __syncthreads();                                          // the last group's rows have been read
        for (int i = t; i < row_words; i += NEIGHBOR_VOTE_BLOCK) rows[i] = 0;
        if (t < G) {                                              // the rows beyond B never have a member
            KdeQuery q;
            q.lat = q.lon = q.thr = q.two_h2 = __builtin_nan("");
            q.cs = q.pad = 0.0;
            if (t < live) {
                q.lon = a.q[2 * (b0 + t)];
                q.lat = a.q[2 * (b0 + t) + 1];
                q.cs = HAV ? cos(q.lat) : 0.0;
                q.thr = a.thr[b0 + t];
                q.two_h2 = a.two_h2[b0 + t];
            }
            qs[t] = q;
        }
        __syncthreads();
        // neighbor_vote_kernel's walk: NEIGHBOR_VOTE_SUBS tiles side by side, NEIGHBOR_UNROLL trips' loads together
        const int sub = t / NEIGHBOR_BLOCK, tt = t % NEIGHBOR_BLOCK;
        for (int64_t tile0 = blockIdx.y; tile0 < a.n_tiles; tile0 += (int64_t)NEIGHBOR_UNROLL * NEIGHBOR_VOTE_SUBS * gridDim.y) {
            NeighborPoint p[NEIGHBOR_UNROLL];
            int64_t j[NEIGHBOR_UNROLL];
#pragma unroll
            for (int u = 0; u < NEIGHBOR_UNROLL; ++u) {
                const int64_t tile = tile0 + (int64_t)(u * NEIGHBOR_VOTE_SUBS + sub) * gridDim.y;
                j[u] = tile < a.n_tiles ? tile * NEIGHBOR_BLOCK + tt : a.M;
                if (j[u] < a.M) p[u] = a.pts[j[u]];
            }
#pragma unroll
            for (int u = 0; u < NEIGHBOR_UNROLL; ++u) {
                if (j[u] < a.M) {
                    for (int g = 0; g < live; ++g) {
                        const KdeQuery& q = qs[g];
                        const double red = neighbor_red<HAV>(q.lon, q.lat, q.cs, p[u].lon, p[u].lat, p[u].cs);
                        if (red <= q.thr) {
                            const uint64_t v = kde_fixed(kde_dist<HAV>(q, p[u], red), q.two_h2, a.scale);
                            atomicAdd(reinterpret_cast<unsigned long long*>(&rows[g * C + p[u].cls]),
                                      (unsigned long long)((uint64_t)(uint32_t)p[u].cell * v));
                        }
                    }
                }
            }
        }
        __syncthreads();
        if (gridDim.y > 1) {
            uint64_t* const out = a.ws + ((int64_t)blockIdx.y * a.groups + grp) * row_words;
            for (int i = t; i < row_words; i += NEIGHBOR_VOTE_BLOCK) out[i] = rows[i];
        } else {
            kde_rank_group(a, rows, b0, live);
        }
    }
}

// the chunks' partial rows of a group, added in LDS, then ranked as the unsplit scan ranks them
__global__ __launch_bounds__(NEIGHBOR_VOTE_BLOCK) void kde_fold_kernel(KdeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t kde_lds[];
    const int t = threadIdx.x;
    const int G = a.G, C = a.C;
    const int row_words = G * C;
    uint64_t* const rows = kde_lds;
    for (int64_t grp = blockIdx.x; grp < a.groups; grp += gridDim.x) {
        const int64_t b0 = grp * G;
        const int live = a.B - b0 < G ? (int)(a.B - b0) : G;
        __syncthreads();
        for (int i = t; i < row_words; i += NEIGHBOR_VOTE_BLOCK) {
            uint64_t n = 0;
            for (int y = 0; y < a.chunks; ++y) n += a.ws[((int64_t)y * a.groups + grp) * row_words + i];
            rows[i] = n;
        }
        __syncthreads();
        kde_rank_group(a, rows, b0, live);
    }
}

}  // namespace range_hip
