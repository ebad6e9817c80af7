// Host side of the cluster map (include/range_cluster.h): argument checks, launches by range_host::cluster_plan and
// the loop over the linkage rounds.  Part of probe_hip.hip (it needs range_probe_ctx and the GEMM launcher).
#pragma once
#include <chrono>

#include "../../include/range_cluster.h"
#include "cluster_kernels.h"
#include "host_plan.h"

namespace {

using range_host::ClusterPlan;
using range_host::cluster_plan;

static_assert(RANGE_CLUSTER_MAX_ROWS == range_host::CLUSTER_MAX_ROWS, "range_cluster.h and host_plan.h disagree");

// the linkage state inside the context's workspace
struct ClusterState {
    uint8_t *active, *stale, *mrow;
    int32_t *nn, *list, *pi, *pj, *counters;
    double* nnd;
};

inline ClusterState cluster_state(uint8_t* ws, const ClusterPlan& p) {
    ClusterState s;
    s.active = ws + p.off_active;
    s.stale = ws + p.off_stale;
    s.mrow = ws + p.off_mrow;
    s.nn = reinterpret_cast<int32_t*>(ws + p.off_nn);
    s.nnd = reinterpret_cast<double*>(ws + p.off_nnd);
    s.list = reinterpret_cast<int32_t*>(ws + p.off_list);
    s.pi = reinterpret_cast<int32_t*>(ws + p.off_pi);
    s.pj = reinterpret_cast<int32_t*>(ws + p.off_pj);
    s.counters = reinterpret_cast<int32_t*>(ws + p.off_counters);
    return s;
}

}  // namespace

extern "C" {

int range_cluster_plan(int64_t n, int32_t d, int64_t max_grid, int64_t* out) {
    if (!out) return fail(RANGE_ERR_INVALID, "null argument");
    const ClusterPlan p = cluster_plan(n, d, max_grid);
    if (!p.valid) return fail(RANGE_ERR_INVALID, "no cluster plan for n=%lld d=%d max_grid=%lld", (long long)n, d,
                              (long long)max_grid);
    out[0] = (int64_t)p.matrix_bytes; out[1] = (int64_t)p.ws_bytes; out[2] = p.norm_grid; out[3] = p.fin_items;
    out[4] = p.fin_grid; out[5] = p.scan_grid; out[6] = p.chunks; out[7] = p.serial_rows;
    return RANGE_OK;
}

int range_cluster_reserve(range_probe_ctx* ctx, int64_t n, int32_t d) {
    if (!ctx) return fail(RANGE_ERR_INVALID, "null argument");
    const ClusterPlan p = cluster_plan(n, d, 0);
    if (!p.valid) return fail(RANGE_ERR_INVALID, "no cluster plan for n=%lld d=%d", (long long)n, d);
    DeviceGuard g(ctx->device);
    HIP_TRY(ctx->ws_cluster.ensure(p.ws_bytes));
    // the split-K slabs E E^T would take (few tiles, d >= 1024)
    const int tiles_m = cdiv(n, GEMM_TILE);
    int k_chunk;
    const int splits = gemm_splits(ctx, tiles_m * (tiles_m + 1) / 2, d, 1, k_chunk);
    if (splits > 1) HIP_TRY(ctx->ws_slabs.ensure((size_t)splits * n * n));
    return RANGE_OK;
}

int range_cluster_normalize(range_probe_ctx* ctx, const double* X, int64_t n, int32_t d, int64_t ldx,
                            const double* mask, double* E, int64_t lde, double* norm2, int64_t max_grid,
                            range_stream_t stream) {
    if (!ctx || !X || !E) return fail(RANGE_ERR_INVALID, "null argument");
    const ClusterPlan p = cluster_plan(n, d, max_grid);
    if (!p.valid || ldx < d || lde < d)
        return fail(RANGE_ERR_INVALID, "bad normalise shape n=%lld d=%d ldx=%lld lde=%lld", (long long)n, d,
                    (long long)ldx, (long long)lde);
    DeviceGuard g(ctx->device);
    hipLaunchKernelGGL(range_cluster::cluster_normalize_kernel, dim3(p.norm_grid), dim3(p.block), 0,
                       (hipStream_t)stream, X, n, d, ldx, mask, E, lde, norm2, p.norm_groups);
    HIP_TRY(hipGetLastError());
    return RANGE_OK;
}

int range_cluster_distances(range_probe_ctx* ctx, const double* E, int64_t n, int32_t d, int64_t lde, double* D,
                            int64_t ldd, int64_t max_grid, range_stream_t stream) {
    if (!ctx || !E || !D) return fail(RANGE_ERR_INVALID, "null argument");
    const ClusterPlan p = cluster_plan(n, d, max_grid);
    if (!p.valid || n < 2 || lde < d || ldd < n)
        return fail(RANGE_ERR_INVALID, "bad distance shape n=%lld d=%d lde=%lld ldd=%lld", (long long)n, d,
                    (long long)lde, (long long)ldd);
    const int tiles_m = cdiv(n, GEMM_TILE);
    int k_chunk;
    const int splits = gemm_splits(ctx, tiles_m * (tiles_m + 1) / 2, d, 1, k_chunk);
    if (splits > 1 && ctx->ws_slabs.n < (size_t)splits * n * n)
        return fail(RANGE_ERR_INVALID, "range_cluster_reserve(n=%lld, d=%d) has not been called", (long long)n, d);
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    // S = E E^T, the tiles on or below the diagonal
    GemmArgs a = gemm_args((int)n, (int)n, d, 1.0, E, lde, 1, E, 1, lde, 0.0, D, ldd);
    a.lower_only = 1;
    const int rc = launch_gemm(ctx, a, true, true, 1, s);
    if (rc) return rc;
    hipLaunchKernelGGL(range_cluster::cluster_finish_kernel, dim3(p.fin_grid), dim3(p.block), 0, s, D, n, ldd,
                       p.fin_items);
    HIP_TRY(hipGetLastError());
    return RANGE_OK;
}

int range_cluster_linkage(range_probe_ctx* ctx, double* D, int64_t n, int64_t ldd, int32_t* merges,
                          double* heights, int32_t* rounds_host, int64_t max_grid, range_stream_t stream) {
    if (!ctx || !D || !merges || !heights) return fail(RANGE_ERR_INVALID, "null argument");
    const ClusterPlan p = cluster_plan(n, 1, max_grid);
    if (!p.valid || n < 2 || ldd < n)
        return fail(RANGE_ERR_INVALID, "bad linkage shape n=%lld ldd=%lld", (long long)n, (long long)ldd);
    if (ctx->ws_cluster.n < p.ws_bytes)
        return fail(RANGE_ERR_INVALID, "range_cluster_reserve(n=%lld) has not been called: the linkage needs %zu "
                    "workspace bytes, the context holds %zu", (long long)n, p.ws_bytes, ctx->ws_cluster.n);
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    const ClusterState st = cluster_state(ctx->ws_cluster.p, p);
    const int32_t n32 = (int32_t)n, per = (int32_t)p.serial_rows, chunks = (int32_t)p.chunks;
    HIP_TRY(hipMemsetAsync(st.active, 1, (size_t)n, s));
    HIP_TRY(hipMemsetAsync(st.mrow, 0, (size_t)n, s));
    HIP_TRY(hipMemsetAsync(st.counters, 0, 64, s));
    int64_t done = 0, rounds = 0;
    using clock = std::chrono::steady_clock;
    const auto ms_since = [](clock::time_point t) { return std::chrono::duration<double, std::milli>(clock::now() - t).count(); };
    const clock::time_point t0 = clock::now();
    clock::time_point t1 = t0;
    ctx->cluster_ms[0] = ctx->cluster_ms[1] = 0.0;
    // every round merges at least one pair: at most n - 1 rounds
    while (done < n - 1 && rounds < n - 1) {
        hipLaunchKernelGGL(range_cluster::cluster_update_list_kernel, dim3(1), dim3(p.serial_block), 0, s, n32, per,
                           (int32_t)(rounds == 0), st.active, st.stale, st.mrow, st.nn, st.list, st.counters);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(range_cluster::cluster_scan_kernel, dim3(p.grid_of(n - done)), dim3(p.block), 0, s, D, ldd,
                           n32, st.active, st.list, st.counters, st.nn, st.nnd);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(range_cluster::cluster_pairs_kernel, dim3(1), dim3(p.serial_block), 0, s, n32, per,
                           st.active, st.nn, st.nnd, st.mrow, st.pi, st.pj, st.counters, merges, heights);
        HIP_TRY(hipGetLastError());
        int32_t pairs = 0;
        HIP_TRY(hipMemcpyAsync(&pairs, st.counters + 1, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (++rounds == 1) {
            ctx->cluster_ms[0] = ms_since(t0);
            t1 = clock::now();
        }
        ctx->cluster_ms[1] = ms_since(t1);
        // impossible under the (distance, index) order - the lexicographically first closest pair is reciprocal -
        // unless the matrix is not symmetric or holds NaN
        if (pairs <= 0 || pairs > n - 1 - done) {
            if (rounds_host) *rounds_host = (int32_t)rounds;
            return fail(RANGE_ERR_INTERNAL, "linkage round %lld found %d reciprocal pairs with %lld clusters left "
                        "(a distance matrix that is not symmetric, or holds NaN?)", (long long)rounds, pairs,
                        (long long)(n - done));
        }
        done += pairs;
        if (done == n - 1) break;                      // one cluster left: nothing reads the merged matrix
        hipLaunchKernelGGL(range_cluster::cluster_merge_rows_kernel, dim3(p.grid_of((int64_t)pairs * chunks)),
                           dim3(p.block), 0, s, D, ldd, n32, st.pi, st.pj, pairs, chunks);
        HIP_TRY(hipGetLastError());
        if (pairs > 1) {
            hipLaunchKernelGGL(range_cluster::cluster_merge_cols_kernel, dim3(p.grid_of(pairs)), dim3(p.block), 0, s,
                               D, ldd, st.pi, st.pj, pairs);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(range_cluster::cluster_mirror_kernel, dim3(p.grid_of((int64_t)pairs * chunks)),
                           dim3(p.block), 0, s, D, ldd, n32, st.active, st.mrow, st.pi, pairs, chunks);
        HIP_TRY(hipGetLastError());
    }
    if (rounds_host) *rounds_host = (int32_t)rounds;
    if (done != n - 1) return fail(RANGE_ERR_INTERNAL, "linkage ended with %lld of %lld merges", (long long)done,
                                   (long long)(n - 1));
    return RANGE_OK;
}

int range_cluster_stage_times(range_probe_ctx* ctx, double* out) {
    if (!ctx || !out) return fail(RANGE_ERR_INVALID, "null argument");
    out[0] = ctx->cluster_ms[0];
    out[1] = ctx->cluster_ms[1];
    return RANGE_OK;
}

int range_cluster_cut(int64_t n, const int32_t* merges_host, const double* heights_host, int64_t n_clusters,
                      int32_t* labels_host, double* Z_host) {
    if (!range_host::cluster_cut(n, merges_host, heights_host, n_clusters, labels_host, Z_host))
        return fail(RANGE_ERR_INVALID, "bad cut: n=%lld n_clusters=%lld, or a merge record that is no tree",
                    (long long)n, (long long)n_clusters);
    return RANGE_OK;
}

}  // extern "C"
