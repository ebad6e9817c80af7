// Device side of the cluster map (include/range_cluster.h; reference: location_models/csp/main/analysis.py:386-434,
// i.e. scikit-learn's AgglomerativeClustering(metric="cosine", linkage="complete") on L2-normalised embeddings).
// All arithmetic is float64.  The pieces:
//   * cluster_normalize_kernel: E = y / |y| with the optional row mask and zero fill, |y|^2 beside it;
//   * cluster_finish_kernel: D = max(0, 1 - S) from the lower triangle of S = E E^T (range_probe_gemm), mirrored so
//     that D[i][j] and D[j][i] are the same bits, +inf on the diagonal - in place;
//   * the linkage rounds.  Complete linkage is reducible, so all mutually nearest pairs of clusters merge in one
//     round: cluster_update_list_kernel (deactivate last round's j's, mark and list the stale rows),
//     cluster_scan_kernel (nearest active neighbour of every stale row under the order (distance, index)),
//     cluster_pairs_kernel (the reciprocal pairs, ascending, into the merge record), then the merge in three
//     launches - cluster_merge_rows_kernel (A: row i <- max(row i, row j)), cluster_merge_cols_kernel (B: inside a
//     merged row, fold the columns of every other pair), cluster_mirror_kernel (C: row i into column i).
// No kernel waits on another workgroup, and within a launch no workgroup reads what another one writes: A writes rows
// i and reads rows j (a row is in at most one pair); B reads and writes its own row i; C reads its own row i and
// writes column i in rows that are not merged this round (D[i'][i] of another merged row i' is already right after A
// and B: max is exact, so both orders of the four-way maximum give the same bits).  Stream order between launches is
// the barrier; the loop over rounds is host code (cluster_host.h).  The launch geometry is
// range_host::cluster_plan (host_plan.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_plan.h"

namespace range_cluster {

using range_host::CLUSTER_BLOCK;
using range_host::CLUSTER_CHUNK;
using range_host::CLUSTER_NORM_REGS;
using range_host::CLUSTER_NORM_ROWS;
using range_host::CLUSTER_SERIAL_BLOCK;
using range_host::CLUSTER_TILE;

constexpr int CLUSTER_WAVES = CLUSTER_BLOCK / 64;
enum { CLUSTER_KEPT = 1, CLUSTER_GONE = 2 };          // mrow: the i and the j of a pair of this round

// ------------------------------------------------------------------------------------------
// E[i, :] = y / |y|_2 and norm2[i] = |y|^2 with y = X[i, :] (mask null), or y = X[i, :] * mask[i] with sqrt(1 / d)
// added to every entry that is then zero (analysis.py:417-423: the fill belongs to the mask).  A wave a row; lane l
// owns columns l, l + 64, ...: up to CLUSTER_NORM_REGS of them stay in registers, so a row of d <= 2048 is read
// once; a wider row is read a second time (from cache).  |y|^2: a lane adds its columns in order, the wave by the
// xor butterfly (every lane ends with the same bits).
__global__ __launch_bounds__(CLUSTER_BLOCK) void cluster_normalize_kernel(const double* __restrict__ X, int64_t n,
                                                                          int32_t d, int64_t ldx,
                                                                          const double* __restrict__ mask,
                                                                          double* __restrict__ E, int64_t lde,
                                                                          double* __restrict__ norm2,
                                                                          int64_t groups) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double fill = sqrt(1.0 / (double)d);
    const bool kept = d <= 64 * CLUSTER_NORM_REGS;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t row = g * CLUSTER_NORM_ROWS + w;
        if (row >= n) continue;                        // (no barrier in this kernel)
        const double* x = X + row * ldx;
        const double m = mask ? mask[row] : 1.0;
        double v[CLUSTER_NORM_REGS];
        double s = 0.0;
        auto entry = [&](int col) {
            double y = x[col];
            if (mask) {
                y *= m;
                if (y == 0.0) y += fill;
            }
            return y;
        };
        if (kept) {
#pragma unroll
            for (int t = 0; t < CLUSTER_NORM_REGS; ++t) {
                const int col = lane + 64 * t;
                v[t] = col < d ? entry(col) : 0.0;
                s = fma(v[t], v[t], s);
            }
        } else {
            for (int col = lane; col < d; col += 64) {
                const double y = entry(col);
                s = fma(y, y, s);
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        const double nrm = sqrt(s);
        double* e = E + row * lde;
        if (kept) {
#pragma unroll
            for (int t = 0; t < CLUSTER_NORM_REGS; ++t) {
                const int col = lane + 64 * t;
                if (col < d) e[col] = v[t] / nrm;
            }
        } else {
            for (int col = lane; col < d; col += 64) e[col] = entry(col) / nrm;
        }
        if (lane == 0 && norm2) norm2[row] = s;
    }
}

// ------------------------------------------------------------------------------------------
// D = max(0, 1 - S) in place (S: the tiles on or below the diagonal hold E E^T).  A workgroup takes tile (ti, tj <= ti)
// of 64 x 64 through LDS: it writes the tile itself and, transposed, tile (tj, ti); on a diagonal tile the entries above
// the diagonal come from below it and the diagonal is +inf.  A NaN stays a NaN.
__global__ __launch_bounds__(CLUSTER_BLOCK) void cluster_finish_kernel(double* __restrict__ D, int64_t n, int64_t ldd,
                                                                       int64_t items) {
    __shared__ double sh[CLUSTER_TILE][CLUSTER_TILE + 1];
    constexpr int PER = CLUSTER_TILE * CLUSTER_TILE / CLUSTER_BLOCK;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        int64_t ti, tj;
        range_host::cluster_tile_of(it, ti, tj);
        const int64_t i0 = ti * CLUSTER_TILE, j0 = tj * CLUSTER_TILE;
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            const int idx = e * CLUSTER_BLOCK + threadIdx.x;
            const int r = idx / CLUSTER_TILE, c = idx % CLUSTER_TILE;
            double v = 0.0;
            if (i0 + r < n && j0 + c < n) {
                v = 1.0 - D[(i0 + r) * ldd + j0 + c];
                v = v < 0.0 ? 0.0 : v;
            }
            sh[r][c] = v;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            const int idx = e * CLUSTER_BLOCK + threadIdx.x;
            const int r = idx / CLUSTER_TILE, c = idx % CLUSTER_TILE;
            if (ti != tj) {
                if (i0 + r < n && j0 + c < n) D[(i0 + r) * ldd + j0 + c] = sh[r][c];
                if (j0 + r < n && i0 + c < n) D[(j0 + r) * ldd + i0 + c] = sh[c][r];
            } else if (i0 + r < n && i0 + c < n) {
                D[(i0 + r) * ldd + i0 + c] = r > c ? sh[r][c] : (r < c ? sh[c][r] : (double)INFINITY);
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// the order of the nearest-neighbour search: (distance, then lower index); k < 0 is "none yet"
__device__ inline bool cluster_closer(double d, int k, double bd, int bk) {
    return k >= 0 && (bk < 0 || d < bd || (d == bd && k < bk));
}

// exclusive prefix sum of one int a thread over the CLUSTER_SERIAL_BLOCK threads of the workgroup; *total = the sum
__device__ inline int cluster_block_scan(int v, int* total) {
    __shared__ int wave_sum[CLUSTER_SERIAL_BLOCK / 64];
    __shared__ int all;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(inc, off, 64);
        if (lane >= off) inc += up;
    }
    __syncthreads();                                   // (an earlier call's reads of wave_sum are done)
    if (lane == 63) wave_sum[w] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int i = 0; i < CLUSTER_SERIAL_BLOCK / 64; ++i) {
            const int t = wave_sum[i];
            wave_sum[i] = run;
            run += t;
        }
        all = run;
    }
    __syncthreads();
    *total = all;
    return wave_sum[w] + inc - v;
}

// (e) of the last round and (a) of this one, one workgroup.  mrow holds the last round's pairs: a j is deactivated,
// an i is stale, and so is every active row whose nearest neighbour was an i or a j; a row whose neighbour is
// untouched keeps it (under complete linkage the distance to a merged cluster only grows).  first != 0: every row
// is stale.  Then mrow is cleared and the stale rows are listed in ascending order.
__global__ __launch_bounds__(CLUSTER_SERIAL_BLOCK) void cluster_update_list_kernel(int32_t n, int32_t per, int32_t first,
                                                                                   uint8_t* __restrict__ active,
                                                                                   uint8_t* __restrict__ stale,
                                                                                   uint8_t* __restrict__ mrow,
                                                                                   const int32_t* __restrict__ nn,
                                                                                   int32_t* __restrict__ list,
                                                                                   int32_t* __restrict__ counters) {
    const int lo = min(n, (int)threadIdx.x * per), hi = min(n, lo + per);
    int cnt = 0;
    for (int r = lo; r < hi; ++r) {
        uint8_t a = active[r], s = a;
        if (!first) {
            const uint8_t m = mrow[r];
            if (m == CLUSTER_GONE) a = 0;
            const int32_t k = nn[r];
            s = a && (m == CLUSTER_KEPT || (k >= 0 && k < n && mrow[k] != 0));
            active[r] = a;
        }
        stale[r] = s;
        cnt += s;
    }
    int total;
    int off = cluster_block_scan(cnt, &total);         // (its barriers: every read of mrow above is done)
    for (int r = lo; r < hi; ++r) {
        mrow[r] = 0;
        if (stale[r]) list[off++] = r;
    }
    if (threadIdx.x == 0) counters[0] = total;
}

// (b) nn[i], nnd[i] of every listed row i: a workgroup scans the row's n doubles coalesced, skips inactive columns
// and i itself, and reduces to the (distance, index) minimum - thread, wave (butterfly), workgroup.
__global__ __launch_bounds__(CLUSTER_BLOCK) void cluster_scan_kernel(const double* __restrict__ D, int64_t ldd, int32_t n,
                                                                     const uint8_t* __restrict__ active,
                                                                     const int32_t* __restrict__ list,
                                                                     const int32_t* __restrict__ counters,
                                                                     int32_t* __restrict__ nn,
                                                                     double* __restrict__ nnd) {
    __shared__ double sd[CLUSTER_WAVES];
    __shared__ int sk[CLUSTER_WAVES];
    constexpr int U = 4;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int cnt = counters[0];
    for (int it = blockIdx.x; it < cnt; it += gridDim.x) {
        const int i = list[it];
        const double* __restrict__ row = D + (int64_t)i * ldd;
        double bd = INFINITY;
        int bk = -1;
        for (int k0 = threadIdx.x; k0 < n; k0 += CLUSTER_BLOCK * U) {
            double v[U];
            uint8_t a[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = k0 + u * CLUSTER_BLOCK;
                const bool ok = k < n;
                v[u] = ok ? row[k] : 0.0;
                a[u] = ok ? active[k] : (uint8_t)0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = k0 + u * CLUSTER_BLOCK;
                if (a[u] && k != i && cluster_closer(v[u], k, bd, bk)) { bd = v[u]; bk = k; }
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double od = __shfl_xor(bd, off, 64);
            const int ok = __shfl_xor(bk, off, 64);
            if (cluster_closer(od, ok, bd, bk)) { bd = od; bk = ok; }
        }
        if (lane == 0) { sd[w] = bd; sk[w] = bk; }
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int x = 1; x < CLUSTER_WAVES; ++x)
                if (cluster_closer(sd[x], sk[x], bd, bk)) { bd = sd[x]; bk = sk[x]; }
            nn[i] = bk;
            nnd[i] = bd;
        }
        __syncthreads();
    }
}

// (c) the reciprocal pairs nn[nn[i]] == i, i < nn[i], in ascending i: into the pair list, the merge record
// (i, j, D[i][j]) behind the merges so far, and mrow.  counters: [0] stale rows, [1] pairs of this round, [2] merges
// so far.  One workgroup.
__global__ __launch_bounds__(CLUSTER_SERIAL_BLOCK) void cluster_pairs_kernel(int32_t n, int32_t per,
                                                                             const uint8_t* __restrict__ active,
                                                                             const int32_t* __restrict__ nn,
                                                                             const double* __restrict__ nnd,
                                                                             uint8_t* __restrict__ mrow,
                                                                             int32_t* __restrict__ pi,
                                                                             int32_t* __restrict__ pj,
                                                                             int32_t* __restrict__ counters,
                                                                             int32_t* __restrict__ merges,
                                                                             double* __restrict__ heights) {
    const int lo = min(n, (int)threadIdx.x * per), hi = min(n, lo + per);
    auto partner = [&](int r) {                         // j of the pair (r, j), or -1
        if (!active[r]) return -1;
        const int j = nn[r];
        return (j > r && j < n && active[j] && nn[j] == r) ? j : -1;
    };
    int cnt = 0;
    for (int r = lo; r < hi; ++r) cnt += partner(r) >= 0;
    const int base = counters[2];
    int total;
    int off = cluster_block_scan(cnt, &total);
    for (int r = lo; r < hi; ++r) {
        const int j = partner(r);
        if (j < 0) continue;
        pi[off] = r;
        pj[off] = j;
        if (base + off < n - 1) {
            merges[2 * (base + off)] = r;
            merges[2 * (base + off) + 1] = j;
            heights[base + off] = nnd[r];
        }
        mrow[r] = CLUSTER_KEPT;
        mrow[j] = CLUSTER_GONE;
        ++off;
    }
    if (threadIdx.x == 0) {
        counters[1] = total;
        counters[2] = base + total;
    }
}

// (d) A: D[i][k] <- max(D[i][k], D[j][k]) for every pair (i, j) and column k; an item is (pair, chunk of columns).
__global__ __launch_bounds__(CLUSTER_BLOCK) void cluster_merge_rows_kernel(double* __restrict__ D, int64_t ldd, int32_t n,
                                                                           const int32_t* __restrict__ pi,
                                                                           const int32_t* __restrict__ pj,
                                                                           int32_t pairs, int32_t chunks) {
    const int64_t items = (int64_t)pairs * chunks;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int t = (int)(it / chunks), c = (int)(it % chunks);
        double* __restrict__ ri = D + (int64_t)pi[t] * ldd;
        const double* __restrict__ rj = D + (int64_t)pj[t] * ldd;
        const int k1 = min(n, (c + 1) * CLUSTER_CHUNK);
        for (int k = c * CLUSTER_CHUNK + threadIdx.x; k < k1; k += CLUSTER_BLOCK) {
            const double a = ri[k], b = rj[k];
            if (b > a) ri[k] = b;
        }
    }
}

// (d) B: inside merged row i, D[i][k] <- max(D[i][k], D[i][l]) for every other pair (k, l) of the round.
__global__ __launch_bounds__(CLUSTER_BLOCK) void cluster_merge_cols_kernel(double* __restrict__ D, int64_t ldd,
                                                                           const int32_t* __restrict__ pi,
                                                                           const int32_t* __restrict__ pj,
                                                                           int32_t pairs) {
    for (int t = blockIdx.x; t < pairs; t += gridDim.x) {
        double* row = D + (int64_t)pi[t] * ldd;
        for (int u = threadIdx.x; u < pairs; u += CLUSTER_BLOCK) {
            if (u == t) continue;
            const int k = pi[u], l = pj[u];
            const double a = row[k], b = row[l];
            if (b > a) row[k] = b;
        }
    }
}

// (d) C: D[k][i] <- D[i][k] for every active row k that is not merged this round, and +inf back on D[i][i]; an item
// is (pair, chunk of rows).
__global__ __launch_bounds__(CLUSTER_BLOCK) void cluster_mirror_kernel(double* __restrict__ D, int64_t ldd, int32_t n,
                                                                       const uint8_t* __restrict__ active,
                                                                       const uint8_t* __restrict__ mrow,
                                                                       const int32_t* __restrict__ pi, int32_t pairs,
                                                                       int32_t chunks) {
    const int64_t items = (int64_t)pairs * chunks;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int t = (int)(it / chunks), c = (int)(it % chunks);
        const int i = pi[t];
        const double* row = D + (int64_t)i * ldd;
        const int k1 = min(n, (c + 1) * CLUSTER_CHUNK);
        for (int k = c * CLUSTER_CHUNK + threadIdx.x; k < k1; k += CLUSTER_BLOCK) {
            if (k == i) D[(int64_t)i * ldd + i] = INFINITY;
            else if (active[k] && mrow[k] == 0) D[(int64_t)k * ldd + i] = row[k];
        }
    }
}

}  // namespace range_cluster
