// The location-only baselines of the CSP evaluation (location_models/csp/main/baselines.py: compute_neighbor_prior
// - 'nn_dist', 'nn_knn' - and GridPrior - 'grid'; eval_helper.py: compute_acc_batch), which the reference serves
// with a BallTree query and a dense (num_classes) prior per validation sample.  Here: one scan of the training set
// per group of queries, the class votes of a query as an int32 row of LDS, and per query the three integers of
// csp_rank_kernel.h - no (B, num_classes) matrix unless the caller asks for the priors.
//
// MEMBERSHIP.  Training point j with class y_j votes for y_j in the row of query i when
//   radius : red(i, j) <= thr                   (thr = sin(dist_thresh / 2)^2 or dist_thresh^2, formed by the host)
//   knn    : (red(i, j), j) is among the k smallest pairs of row i under the TOTAL order (red, then index j)
//   cell   : cell(i) == cell(j)                 (int32 ids from the host; a training point outside the grid has -2,
//                                                a query that takes the uniform prior -1)
// red(i, j), float64, nothing contracted, in scikit-learn's expression order:
//   haversine (radians): sin(.5 (lat_i - lat_j))^2 + cos(lat_i) cos(lat_j) sin(.5 (lon_i - lon_j)) sin(.5 (lon_i - lon_j))
//   euclidean (degrees): (lat_i - lat_j)^2 + (lon_i - lon_j)^2
// A NaN red is never a member: a NaN query has no votes, which is the reference's uniform prior for the two
// neighbour priors.  BallTree leaves the choice among equally distant points unspecified; the total order above is
// the rule here, as the order (a, index) is checker_merge_kernel's.
//
// PRIOR AND SCORE.  cnt[c] the votes of a row, n their sum, C the classes, one correctly rounded division each:
//   neighbours : prior[c] = (1.0 + cnt[c]) / (double)(C + n)
//   grid       : prior[c] = ((cnt[c] + pc) - 1.0) / ((n + C pc) - C)        (C pc formed by the host; 0 / 0 is NaN as in numpy)
//                a query with cell -1: 1.0 / C
// score s[c] = (double) img[c] * prior[c], or prior[c] without image predictions; greater / tied_after / argmax and
// their -1 / -2 flags are csp_rank_kernel.h's, by its csp_rank_before.
//
// WORK SPLIT (host_plan.h: neighbor_plan, kde_plan).  One scan (neighbor_vote_body) and one fold (neighbor_fold_body)
// serve every prior here and the KDE prior of kde_kernel.h; a ROW POLICY says what a row holds: the entry type
// (int32 votes, uint64 fixed-point sums), the query's record of NEIGHBOR_QUERY_LDS bytes and how it is loaded, what a
// member adds to its class entry, and the row's statistic behind prior_of.  A workgroup owns G queries, their
// records (wave-uniform LDS reads) and zeroed rows; its 1024 threads walk the packed training points (32 bytes a
// point, cos lat formed once by neighbor_prep_kernel) in tiles of 256, four tiles side by side, each thread its
// point against the G queries; a member costs one LDS integer add.  Integer adds are order-free: the rows depend on
// no split.  With one chunk each wave then ranks rows of the group from LDS; with more, chunk y stores its rows to
// the workspace and the fold adds the chunks in LDS and ranks - the same integers, hence the same bits.
//
// SELECTION.  neighbor_select_kernel, a workgroup a query: the k-th smallest (red, j) by a radix select over the
// key of red - its bit pattern with the sign bit flipped (all bits for a negative value), which orders as red does.
// Every pass rescans the training set with the vote scan's neighbor_red, counts the digit of the keys that share
// the prefix found so far in an LDS histogram and narrows to the bin that holds the k-th.  A last, ordered walk over
// j counts the keys equal to the k-th by ballot and prefix and stops at j_last, the last tie to take.  The vote
// scan's predicate is then red < red_k || (red == red_k && j <= j_last).  Fewer than k pairs with a number for
// red (a NaN query): red_k is NaN, j_last -1, and every pair with a number is a member.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csp_rank_kernel.h"
#include "host_plan.h"

namespace range_hip {

using range_host::NEIGHBOR_BINS;
using range_host::NEIGHBOR_BLOCK;
using range_host::NEIGHBOR_CELL;
using range_host::NEIGHBOR_DIGIT_BITS;
using range_host::NEIGHBOR_KNN;
using range_host::NEIGHBOR_PASSES;
using range_host::NEIGHBOR_RADIUS;
using range_host::NEIGHBOR_VOTE_BLOCK;

constexpr int32_t NEIGHBOR_CELL_UNIFORM = -1, NEIGHBOR_CELL_OUTSIDE = -2;
constexpr int NEIGHBOR_UNROLL = 2;       // trips of the vote scan whose point loads a thread keeps in flight
constexpr int NEIGHBOR_VOTE_SUBS = NEIGHBOR_VOTE_BLOCK / NEIGHBOR_BLOCK;

struct NeighborPoint {       // 32 bytes: two 16-byte loads a lane
    double lat, lon, cs;     // cs = cos(lat) (haversine), else 0
    int32_t cls, cell;
};

struct NeighborQuery {       // NEIGHBOR_QUERY_LDS bytes
    double lat, lon, cs;
    double thr;              // radius: the threshold; knn: red_k
    int64_t j_last;          // knn
    int32_t cell, pad;
};
static_assert(sizeof(NeighborPoint) == 32 && sizeof(NeighborQuery) == range_host::NEIGHBOR_QUERY_LDS, "layout");

// what every row policy's scan and fold take; `raw` (B, C) or null - the rows themselves - and `ws` - chunks > 1:
// (chunks, groups, G * C) partial rows - are of the policy's entry type and stand in its own struct
struct NeighborScanArgs {
    const NeighborPoint* pts;
    int64_t N, n_tiles;
    const double* q;                 // (B, 2) (lon, lat): radians (haversine) or degrees; null in cell mode
    int64_t B, groups;
    int32_t G, C;
    const void* img;                 // (B, C) float32 / float64 or null
    int32_t img_kind;
    const int32_t* labels;           // (B), with greater / tied / argmax
    int32_t *greater, *tied, *argmax;
    double* prior;                   // (B, C) or null
    int32_t chunks;                  // fold: how many
};

struct NeighborArgs : NeighborScanArgs {
    const int32_t* qcell;            // (B), cell mode
    double thr;                      // radius
    const double* red_k;             // (B), knn
    const int64_t* j_last;           // (B), knn
    double pc, cpc;                  // cell: pseudo_count and num_classes * pseudo_count
    int32_t *raw, *ws;               // the votes
};

struct NeighborSelectArgs {
    const NeighborPoint* pts;
    int64_t N;
    const double* q;
    int64_t B, k;
    double* red_k;
    int64_t* j_last;
};

template <bool HAV>
__device__ __forceinline__ double neighbor_red(double lon1, double lat1, double c1, double lon2, double lat2, double c2) {
#pragma clang fp contract(off)
    if (HAV) {
        const double s0 = sin(0.5 * (lat1 - lat2));
        const double s1 = sin(0.5 * (lon1 - lon2));
        const double h = s0 * s0;
        const double cc = c1 * c2;
        const double c1s = cc * s1;
        const double c2s = c1s * s1;
        return h + c2s;
    }
    const double dlat = lat1 - lat2, dlon = lon1 - lon2;
    const double a = dlat * dlat;
    const double b = dlon * dlon;
    return a + b;
}

// orders as the doubles do (-0 below +0; red is never -0: a sum of squares, or of a square and a product)
__device__ __forceinline__ uint64_t neighbor_key(double red) {
    const uint64_t b = (uint64_t)__double_as_longlong(red);
    return b ^ ((b >> 63) ? ~UINT64_C(0) : UINT64_C(0x8000000000000000));
}
__device__ __forceinline__ double neighbor_unkey(uint64_t key) {
    const uint64_t b = key ^ ((key >> 63) ? UINT64_C(0x8000000000000000) : ~UINT64_C(0));
    return __longlong_as_double((long long)b);
}

// the packed training set: lonlat (N, 2) (lon, lat), classes (N), cells (N) or null
__global__ __launch_bounds__(NEIGHBOR_BLOCK) void neighbor_prep_kernel(const double* lonlat, const int32_t* cls, const int32_t* cell,
                                                                       int64_t N, int32_t hav, NeighborPoint* out) {
    for (int64_t j = (int64_t)blockIdx.x * NEIGHBOR_BLOCK + threadIdx.x; j < N; j += (int64_t)gridDim.x * NEIGHBOR_BLOCK) {
        NeighborPoint p;
        p.lon = lonlat[2 * j];
        p.lat = lonlat[2 * j + 1];
        p.cs = hav ? cos(p.lat) : 0.0;
        p.cls = cls[j];
        p.cell = cell ? cell[j] : NEIGHBOR_CELL_OUTSIDE;
        out[j] = p;
    }
}

// the three integers of row b by one wave: the scores are img[b, c] * prior_at(c) (prior_at(c) without image
// predictions), the rule csp_rank_kernel.h's.  Shared by the count priors here and the KDE prior (kde_kernel.h).
template <class PriorAt>
__device__ __forceinline__ void neighbor_rank_row(const void* img, int32_t img_kind, const int32_t* labels, int32_t* greater,
                                                  int32_t* tied, int32_t* argmax, int64_t b, int C, int lane, const PriorAt& prior_at) {
#pragma clang fp contract(off)
    const auto score_of = [&](int c) {
        const double p = prior_at(c);
        if (img_kind == CSP_IMG_F32) return (double)static_cast<const float*>(img)[b * C + c] * p;
        if (img_kind == CSP_IMG_F64) return static_cast<const double*>(img)[b * C + c] * p;
        return p;
    };
    const int32_t label = labels[b];
    const bool bad = label < 0 || label >= C;
    const double st = bad ? 0.0 : score_of(label);
    int32_t ngt = 0, ntie = 0, bi = CSP_RANK_NO_INDEX;
    double bs = -__builtin_inf();
    for (int c = lane; c < C; c += 64) {
        const double s = score_of(c);
        ngt += (c != label && !(s <= st)) ? 1 : 0;
        ntie += (s == st && c > label) ? 1 : 0;
        if (csp_rank_before(s, c, bs, bi)) { bs = s; bi = c; }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        ngt += __shfl_xor(ngt, o);
        ntie += __shfl_xor(ntie, o);
        const double os = __shfl_xor(bs, o);
        const int32_t oi = __shfl_xor(bi, o);
        if (csp_rank_before(os, oi, bs, bi)) { bs = os; bi = oi; }
    }
    if (lane == 0) {
        const int32_t flag = bad ? CSP_RANK_BAD_LABEL : st != st ? CSP_RANK_NAN : 0;
        greater[b] = flag ? flag : ngt;
        tied[b] = flag ? flag : ntie;
        argmax[b] = flag ? flag : bi;
    }
}

// ---- the scan, the fold and the ranks of a group over a row policy P:
//   P::Entry, P::Query (NEIGHBOR_QUERY_LDS bytes), P::Args (NeighborScanArgs and Entry *raw, *ws)
//   P::stage(a, q, b, live)       the record of query b for the scan; !live: a row beyond B, which never has a member
//   P::stage_fold(a, q, b, live)  what of it the ranks read
//   P::member(a, q, p, j, row)    the predicate of point j and the one LDS add to row[p.cls]
//   P::prior_of(a, q, row, lane)  the row's reduction by one wave; returns entry -> prior

// the LDS of a workgroup: the rows, rounded up to 16 bytes, then the G records
template <class Entry>
__device__ __forceinline__ size_t neighbor_query_offset(int row_entries) {
    return ((size_t)row_entries * sizeof(Entry) + 15) & ~(size_t)15;
}

// the rows of a group, a wave each (rows wave, wave + 16, ...): raw rows / priors on request, the three integers
template <class P>
__device__ __forceinline__ void neighbor_rank_group(const typename P::Args& a, const typename P::Entry* rows,
                                                    const typename P::Query* qs, int64_t b0, int live) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int C = a.C;
    for (int g = wave; g < live; g += NEIGHBOR_VOTE_BLOCK / 64) {
        const typename P::Entry* const row = rows + (size_t)g * C;
        const int64_t b = b0 + g;
        const auto prior_of = P::prior_of(a, qs[g], row, lane);
        if (a.raw)
            for (int c = lane; c < C; c += 64) a.raw[b * C + c] = row[c];
        if (a.prior)
            for (int c = lane; c < C; c += 64) a.prior[b * C + c] = prior_of(row[c]);
        if (!a.greater) continue;
        neighbor_rank_row(a.img, a.img_kind, a.labels, a.greater, a.tied, a.argmax, b, C, lane, [&](int c) { return prior_of(row[c]); });
    }
}

template <class P>
__device__ __forceinline__ void neighbor_vote_body(const typename P::Args& a) {
    using Entry = typename P::Entry;
    extern __shared__ __attribute__((aligned(16))) unsigned char neighbor_lds[];
    const int t = threadIdx.x;
    const int G = a.G, C = a.C;
    const int row_entries = G * C;                                // at most NEIGHBOR_COUNT_LDS / sizeof(Entry)
    Entry* const rows = reinterpret_cast<Entry*>(neighbor_lds);
    typename P::Query* const qs = reinterpret_cast<typename P::Query*>(neighbor_lds + neighbor_query_offset<Entry>(row_entries));
    for (int64_t grp = blockIdx.x; grp < a.groups; grp += gridDim.x) {
        const int64_t b0 = grp * G;
        const int live = a.B - b0 < G ? (int)(a.B - b0) : G;
        __syncthreads();                                          // the last group's rows have been read
        for (int i = t; i < row_entries; i += NEIGHBOR_VOTE_BLOCK) rows[i] = 0;
        if (t < G) P::stage(a, qs[t], b0 + t, t < live);
        __syncthreads();
        // The workgroup is NEIGHBOR_VOTE_BLOCK threads: NEIGHBOR_VOTE_SUBS tiles of NEIGHBOR_BLOCK points side by side,
        // NEIGHBOR_UNROLL such trips' loads issued together.  The rows leave room for one workgroup a CU at the
        // widest rows: four waves a SIMD of ONE workgroup hide the latency of the float64 chains, four workgroups of
        // 256 would need four times the rows.
        const int sub = t / NEIGHBOR_BLOCK, tt = t % NEIGHBOR_BLOCK;
        for (int64_t tile0 = blockIdx.y; tile0 < a.n_tiles; tile0 += (int64_t)NEIGHBOR_UNROLL * NEIGHBOR_VOTE_SUBS * gridDim.y) {
            NeighborPoint p[NEIGHBOR_UNROLL];
            int64_t j[NEIGHBOR_UNROLL];
#pragma unroll
            for (int u = 0; u < NEIGHBOR_UNROLL; ++u) {
                const int64_t tile = tile0 + (int64_t)(u * NEIGHBOR_VOTE_SUBS + sub) * gridDim.y;
                j[u] = tile < a.n_tiles ? tile * NEIGHBOR_BLOCK + tt : a.N;
                if (j[u] < a.N) p[u] = a.pts[j[u]];
            }
#pragma unroll
            for (int u = 0; u < NEIGHBOR_UNROLL; ++u) {
                if (j[u] < a.N) {
                    for (int g = 0; g < live; ++g) P::member(a, qs[g], p[u], j[u], rows + g * C);
                }
            }
        }
        __syncthreads();
        if (gridDim.y > 1) {
            Entry* const out = a.ws + ((int64_t)blockIdx.y * a.groups + grp) * row_entries;
            for (int i = t; i < row_entries; i += NEIGHBOR_VOTE_BLOCK) out[i] = rows[i];
        } else {
            neighbor_rank_group<P>(a, rows, qs, b0, live);
        }
    }
}

// the chunks' partial rows of a group, added in LDS, then ranked as the unsplit scan ranks them
template <class P>
__device__ __forceinline__ void neighbor_fold_body(const typename P::Args& a) {
    using Entry = typename P::Entry;
    extern __shared__ __attribute__((aligned(16))) unsigned char neighbor_lds[];
    const int t = threadIdx.x;
    const int G = a.G, C = a.C;
    const int row_entries = G * C;
    Entry* const rows = reinterpret_cast<Entry*>(neighbor_lds);
    typename P::Query* const qs = reinterpret_cast<typename P::Query*>(neighbor_lds + neighbor_query_offset<Entry>(row_entries));
    for (int64_t grp = blockIdx.x; grp < a.groups; grp += gridDim.x) {
        const int64_t b0 = grp * G;
        const int live = a.B - b0 < G ? (int)(a.B - b0) : G;
        __syncthreads();
        for (int i = t; i < row_entries; i += NEIGHBOR_VOTE_BLOCK) {
            Entry n = 0;
            for (int y = 0; y < a.chunks; ++y) n += a.ws[((int64_t)y * a.groups + grp) * row_entries + i];
            rows[i] = n;
        }
        if (t < G) P::stage_fold(a, qs[t], b0 + t, t < live);
        __syncthreads();
        neighbor_rank_group<P>(a, rows, qs, b0, live);
    }
}

// ---- the count rows: int32 votes by predicate MODE under metric HAV (the fold and the ranks read MODE alone)
template <int MODE, bool HAV>
struct NeighborCountRows {
    using Entry = int32_t;
    using Query = NeighborQuery;
    using Args = NeighborArgs;

    static __device__ __forceinline__ void stage(const Args& a, Query& out, int64_t b, bool live) {
        Query q;
        q.lat = q.lon = q.thr = __builtin_nan("");
        q.cs = 0.0;
        q.j_last = -1;
        q.cell = NEIGHBOR_CELL_UNIFORM;
        q.pad = 0;
        if (live) {
            if (MODE == NEIGHBOR_CELL) {
                q.cell = a.qcell[b];
            } else {
                q.lon = a.q[2 * b];
                q.lat = a.q[2 * b + 1];
                q.cs = HAV ? cos(q.lat) : 0.0;
                q.thr = MODE == NEIGHBOR_RADIUS ? a.thr : a.red_k[b];
                if (MODE == NEIGHBOR_KNN) q.j_last = a.j_last[b];
            }
        }
        out = q;
    }

    static __device__ __forceinline__ void stage_fold(const Args& a, Query& out, int64_t b, bool live) {
        Query q{};                       // (the ranks read the cell alone)
        q.cell = MODE == NEIGHBOR_CELL && live ? a.qcell[b] : NEIGHBOR_CELL_UNIFORM;
        out = q;
    }

    static __device__ __forceinline__ void member(const Args&, const Query& q, const NeighborPoint& p, int64_t j, Entry* row) {
        bool in;
        if (MODE == NEIGHBOR_CELL) {
            in = p.cell == q.cell;
        } else {
            const double red = neighbor_red<HAV>(q.lon, q.lat, q.cs, p.lon, p.lat, p.cs);
            const double rk = q.thr;
            if (MODE == NEIGHBOR_RADIUS) in = red <= rk;
            else if (rk != rk) in = red == red;                   // fewer than k pairs with a number: all of them
            else in = red < rk || (red == rk && j <= q.j_last);
        }
        if (in) atomicAdd(&row[p.cls], 1);
    }

    static __device__ __forceinline__ auto prior_of(const Args& a, const Query& q, const Entry* row, int lane) {
#pragma clang fp contract(off)
        const int C = a.C;
        int32_t n = 0;
        for (int c = lane; c < C; c += 64) n += row[c];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) n += __shfl_xor(n, o);
        const bool uniform = MODE == NEIGHBOR_CELL && q.cell == NEIGHBOR_CELL_UNIFORM;
        const double den = MODE == NEIGHBOR_CELL ? ((double)n + a.cpc) - (double)C : (double)((int64_t)C + (int64_t)n);
        const double pc = a.pc, one_c = 1.0 / (double)C;
        return [=](int32_t cnt) {
            if (uniform) return one_c;
            if (MODE == NEIGHBOR_CELL) return (((double)cnt + pc) - 1.0) / den;
            return (1.0 + (double)cnt) / den;
        };
    }
};

template <int MODE, bool HAV>
__global__ __launch_bounds__(NEIGHBOR_VOTE_BLOCK) void neighbor_vote_kernel(NeighborArgs a) {
    neighbor_vote_body<NeighborCountRows<MODE, HAV>>(a);
}

template <int MODE>
__global__ __launch_bounds__(NEIGHBOR_VOTE_BLOCK) void neighbor_fold_kernel(NeighborArgs a) {
    neighbor_fold_body<NeighborCountRows<MODE, false>>(a);
}

template <bool HAV>
__global__ __launch_bounds__(NEIGHBOR_BLOCK) void neighbor_select_kernel(NeighborSelectArgs a) {
    __shared__ uint32_t hist[NEIGHBOR_BINS];
    __shared__ uint32_t part[NEIGHBOR_BLOCK];
    __shared__ uint32_t wcnt[NEIGHBOR_BLOCK / 64];
    __shared__ int32_t s_digit;          // -1: fewer than the wanted pairs
    __shared__ int64_t s_rem, s_jlast;
    constexpr int PER = NEIGHBOR_BINS / NEIGHBOR_BLOCK;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
        const double lon1 = a.q[2 * b], lat1 = a.q[2 * b + 1];
        const double c1 = HAV ? cos(lat1) : 0.0;
        uint64_t prefix = 0;
        int64_t rem = a.k;               // the rank of the k-th among the keys that share the prefix
        bool enough = true;
        for (int pass = 0; pass < NEIGHBOR_PASSES; ++pass) {
            const int shift = range_host::NeighborPlan::shift_of(pass);
            __syncthreads();             // the last pass's (query's) reads of hist, part and s_* are done
            for (int i = t; i < NEIGHBOR_BINS; i += NEIGHBOR_BLOCK) hist[i] = 0;
            __syncthreads();
            for (int64_t j = t; j < a.N; j += NEIGHBOR_BLOCK) {
                const NeighborPoint p = a.pts[j];
                const double red = neighbor_red<HAV>(lon1, lat1, c1, p.lon, p.lat, p.cs);
                if (red == red) {
                    const uint64_t key = neighbor_key(red);
                    // (pass 0 has no prefix; its shift + NEIGHBOR_DIGIT_BITS is beyond the key)
                    if (pass == 0 || (key >> (shift + NEIGHBOR_DIGIT_BITS)) == (prefix >> (shift + NEIGHBOR_DIGIT_BITS)))
                        atomicAdd(&hist[(key >> shift) & (NEIGHBOR_BINS - 1)], 1u);
                }
            }
            __syncthreads();
            uint32_t mine = 0;
#pragma unroll
            for (int i = 0; i < PER; ++i) mine += hist[t * PER + i];
            part[t] = mine;
            __syncthreads();
            if (t == 0) {
                int64_t below = 0;
                int32_t digit = -1;
                for (int w = 0; w < NEIGHBOR_BLOCK && digit < 0; ++w) {
                    if (below + part[w] < rem) { below += part[w]; continue; }
                    for (int i = 0; i < PER; ++i) {
                        const uint32_t h = hist[w * PER + i];
                        if (below + h >= rem) { digit = w * PER + i; break; }
                        below += h;
                    }
                }
                s_digit = digit;
                s_rem = rem - below;
            }
            __syncthreads();
            if (s_digit < 0) { enough = false; break; }           // (block-uniform; pass 0 alone can fall short)
            prefix |= (uint64_t)s_digit << shift;
            rem = s_rem;
        }
        if (!enough) {
            if (t == 0) {
                a.red_k[b] = neighbor_unkey(~UINT64_C(0));        // a NaN
                a.j_last[b] = -1;
            }
            continue;
        }
        // the rem-th index, ascending, whose key is the k-th key
        int64_t seen = 0;
        for (int64_t j0 = 0; j0 < a.N; j0 += NEIGHBOR_BLOCK) {
            const int64_t j = j0 + t;
            bool hit = false;
            if (j < a.N) {
                const NeighborPoint p = a.pts[j];
                const double red = neighbor_red<HAV>(lon1, lat1, c1, p.lon, p.lat, p.cs);
                hit = red == red && neighbor_key(red) == prefix;
            }
            const uint64_t m = __ballot(hit);
            __syncthreads();             // the last tile's reads of wcnt are done
            if (lane == 0) wcnt[wave] = (uint32_t)__popcll(m);
            __syncthreads();
            int64_t before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < NEIGHBOR_BLOCK / 64; ++w) {
                before += w < wave ? wcnt[w] : 0;
                total += wcnt[w];
            }
            before += __popcll(m & ((UINT64_C(1) << lane) - 1));
            if (hit && seen + before + 1 == rem) s_jlast = j;
            seen += total;
            if (seen >= rem) break;      // (block-uniform)
        }
        __syncthreads();
        if (t == 0) {
            a.red_k[b] = neighbor_unkey(prefix);
            a.j_last[b] = s_jlast;
        }
    }
}

}  // namespace range_hip
