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
// WORK SPLIT (host_plan.h: kde_plan): neighbor_kernel.h's scan and fold over the row policy KdeRows below (uint64
// rows: half as many queries a workgroup).
#pragma once
#include "neighbor_kernel.h"

namespace range_hip {

struct KdeQuery {            // NEIGHBOR_QUERY_LDS bytes
    double lat, lon, cs;
    double thr, two_h2;
    double pad;
};
static_assert(sizeof(KdeQuery) == range_host::NEIGHBOR_QUERY_LDS, "layout");

struct KdeArgs : NeighborScanArgs {  // (the `cell` of pts is the bin's count, N their number M)
    const double* thr;               // (B)
    const double* two_h2;            // (B)
    double scale;                    // 2^s
    uint64_t *raw, *ws;              // the sums
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

// the KDE rows: uint64 fixed-point sums of the members' weights under metric HAV (the fold and the ranks read no record)
template <bool HAV>
struct KdeRows {
    using Entry = uint64_t;
    using Query = KdeQuery;
    using Args = KdeArgs;

    static __device__ __forceinline__ void stage(const Args& a, Query& out, int64_t b, bool live) {
        Query q;
        q.lat = q.lon = q.thr = q.two_h2 = __builtin_nan("");
        q.cs = q.pad = 0.0;
        if (live) {
            q.lon = a.q[2 * b];
            q.lat = a.q[2 * b + 1];
            q.cs = HAV ? cos(q.lat) : 0.0;
            q.thr = a.thr[b];
            q.two_h2 = a.two_h2[b];
        }
        out = q;
    }

    static __device__ __forceinline__ void stage_fold(const Args&, Query&, int64_t, bool) {}

    static __device__ __forceinline__ void member(const Args& a, const Query& q, const NeighborPoint& p, int64_t, Entry* row) {
        const double red = neighbor_red<HAV>(q.lon, q.lat, q.cs, p.lon, p.lat, p.cs);
        if (red <= q.thr) {
            const uint64_t v = kde_fixed(kde_dist<HAV>(q, p, red), q.two_h2, a.scale);
            atomicAdd(reinterpret_cast<unsigned long long*>(&row[p.cls]), (unsigned long long)((uint64_t)(uint32_t)p.cell * v));
        }
    }

    static __device__ __forceinline__ auto prior_of(const Args& a, const Query&, const Entry* row, int lane) {
#pragma clang fp contract(off)
        const int C = a.C;
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
        return [=](uint64_t v) { return uniform ? one_c : ((double)v + m) / den; };
    }
};

template <bool HAV>
__global__ __launch_bounds__(NEIGHBOR_VOTE_BLOCK) void kde_vote_kernel(KdeArgs a) {
    neighbor_vote_body<KdeRows<HAV>>(a);
}

__global__ __launch_bounds__(NEIGHBOR_VOTE_BLOCK) void kde_fold_kernel(KdeArgs a) {
    neighbor_fold_body<KdeRows<false>>(a);
}

}  // namespace range_hip
