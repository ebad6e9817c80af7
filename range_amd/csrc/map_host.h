// Host side of the embedding map (include/range_map.h): argument checks and launches by range_host::map_plan.
// Part of probe_hip.hip (it needs the definition of range_probe_ctx).
#pragma once
#include "../../include/range_map.h"
#include "host_plan.h"
#include "map_kernels.h"

namespace {

using range_host::MapPlan;
using range_host::map_plan;

static_assert(RANGE_MAP_MAX_C == range_host::MAP_MAX_C && RANGE_MAP_MAX_BINS == range_host::MAP_MAX_BINS,
              "range_map.h and host_plan.h disagree");

// run `body` with C = c as a constant
#define MAP_FOR_C(c, body)                       \
    switch (c) {                                 \
        case 1: { constexpr int C = 1; body; } break; \
        case 2: { constexpr int C = 2; body; } break; \
        case 3: { constexpr int C = 3; body; } break; \
        case 4: { constexpr int C = 4; body; } break; \
        case 5: { constexpr int C = 5; body; } break; \
        case 6: { constexpr int C = 6; body; } break; \
        case 7: { constexpr int C = 7; body; } break; \
        default: { constexpr int C = 8; body; } break; \
    }

inline range_map::MapMat map_mat(const double* host, int c) {
    range_map::MapMat m{};
    for (int i = 0; i < c * c; ++i) m.m[i] = host[i];
    return m;
}

}  // namespace

extern "C" {

int range_map_plan(int64_t n, int32_t c, int64_t max_grid, int64_t* out) {
    if (!out) return fail(RANGE_ERR_INVALID, "null argument");
    const MapPlan p = map_plan(n, c, max_grid);
    if (!p.valid) return fail(RANGE_ERR_INVALID, "no map plan for n=%lld c=%d max_grid=%lld", (long long)n, c,
                              (long long)max_grid);
    out[0] = p.chunk; out[1] = p.slabs; out[2] = p.step_grid; out[3] = (int64_t)p.ws_bytes;
    out[4] = range_host::MAP_PROJ_ROWS; out[5] = p.proj_grid;
    out[6] = p.block; out[7] = p.eq_grid;
    return RANGE_OK;
}

int range_map_reserve(range_probe_ctx* ctx, int64_t n, int32_t c) {
    if (!ctx) return fail(RANGE_ERR_INVALID, "null argument");
    const MapPlan p = map_plan(n, c, 0);
    if (!p.valid) return fail(RANGE_ERR_INVALID, "no map plan for n=%lld c=%d", (long long)n, c);
    DeviceGuard g(ctx->device);
    HIP_TRY(ctx->ws_map.ensure(p.ws_bytes / sizeof(double)));
    return RANGE_OK;
}

int range_map_project(range_probe_ctx* ctx, const double* X, int64_t n, int32_t d, int64_t ldx,
                      const double* mean, const double* K, int32_t c, double* Y, int64_t ldy,
                      int64_t max_grid, range_stream_t stream) {
    if (!ctx || !X || !K || !Y) return fail(RANGE_ERR_INVALID, "null argument");
    const MapPlan p = map_plan(n, c, max_grid);
    if (!p.valid || d <= 0 || ldx < d || ldy < n)
        return fail(RANGE_ERR_INVALID, "bad projection shape n=%lld d=%d c=%d ldx=%lld ldy=%lld", (long long)n, d,
                    c, (long long)ldx, (long long)ldy);
    DeviceGuard g(ctx->device);
    const bool vec = aligned(X, 16) && ldx % 2 == 0;
    MAP_FOR_C(c, {
        if (vec) hipLaunchKernelGGL((range_map::map_project_kernel<C, true>), dim3(p.proj_grid), dim3(p.block), 0,
                                    (hipStream_t)stream, X, n, d, ldx, mean, K, Y, ldy, p.proj_groups);
        else hipLaunchKernelGGL((range_map::map_project_kernel<C, false>), dim3(p.proj_grid), dim3(p.block), 0,
                                (hipStream_t)stream, X, n, d, ldx, mean, K, Y, ldy, p.proj_groups);
    });
    HIP_TRY(hipGetLastError());
    return RANGE_OK;
}

int range_map_ica_step(range_probe_ctx* ctx, const double* Y, int64_t n, int64_t ldy, int32_t c,
                       const double* W_host, double* out, int64_t max_grid, range_stream_t stream) {
    if (!ctx || !Y || !W_host || !out) return fail(RANGE_ERR_INVALID, "null argument");
    const MapPlan p = map_plan(n, c, max_grid);
    if (!p.valid || ldy < n)
        return fail(RANGE_ERR_INVALID, "bad ICA-step shape n=%lld c=%d ldy=%lld", (long long)n, c, (long long)ldy);
    if (ctx->ws_map.n * sizeof(double) < p.ws_bytes)
        return fail(RANGE_ERR_INVALID, "range_map_reserve(n=%lld, c=%d) has not been called: the step needs %zu "
                    "workspace bytes, the context holds %zu", (long long)n, c, p.ws_bytes,
                    ctx->ws_map.n * sizeof(double));
    DeviceGuard g(ctx->device);
    const range_map::MapMat W = map_mat(W_host, c);
    MAP_FOR_C(c, {
        hipLaunchKernelGGL((range_map::map_ica_step_kernel<C>), dim3(p.step_grid), dim3(p.block), 0,
                           (hipStream_t)stream, Y, n, ldy, W, p.ipt, p.slabs, ctx->ws_map.p);
    });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(range_map::map_fold_kernel, dim3(1), dim3(p.block), 0, (hipStream_t)stream,
                       (const double*)ctx->ws_map.p, p.slabs, (int32_t)p.slab_doubles, out);
    HIP_TRY(hipGetLastError());
    return RANGE_OK;
}

int range_map_sources(range_probe_ctx* ctx, const double* Y, int64_t n, int64_t ldy, int32_t c,
                      const double* M_host, double* S, int64_t max_grid, range_stream_t stream) {
    if (!ctx || !Y || !M_host || !S) return fail(RANGE_ERR_INVALID, "null argument");
    const MapPlan p = map_plan(n, c, max_grid);
    if (!p.valid || ldy < n)
        return fail(RANGE_ERR_INVALID, "bad sources shape n=%lld c=%d ldy=%lld", (long long)n, c, (long long)ldy);
    DeviceGuard g(ctx->device);
    const range_map::MapMat M = map_mat(M_host, c);
    MAP_FOR_C(c, {
        hipLaunchKernelGGL((range_map::map_sources_kernel<C>), dim3(p.eq_grid), dim3(p.block), 0,
                           (hipStream_t)stream, Y, n, ldy, M, S);
    });
    HIP_TRY(hipGetLastError());
    return RANGE_OK;
}

int range_map_equalize(range_probe_ctx* ctx, const double* x, int64_t n, int64_t ldx, const double* edges,
                       int32_t nbins, uint64_t* counts, double* out, int64_t ldo, int64_t max_grid,
                       range_stream_t stream) {
    if (!ctx || !x || !edges || !counts || !out) return fail(RANGE_ERR_INVALID, "null argument");
    const MapPlan p = map_plan(n, 1, max_grid);
    if (!p.valid || ldx < 1 || ldo < 1 || nbins < 2 || nbins > RANGE_MAP_MAX_BINS)
        return fail(RANGE_ERR_INVALID, "bad equalisation shape n=%lld nbins=%d (2..%d) ldx=%lld ldo=%lld",
                    (long long)n, nbins, RANGE_MAP_MAX_BINS, (long long)ldx, (long long)ldo);
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    auto* cnt = reinterpret_cast<unsigned long long*>(counts);
    HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * nbins, s));
    hipLaunchKernelGGL(range_map::map_hist_kernel, dim3(p.eq_grid), dim3(p.block), 0, s, x, n, ldx, edges, nbins,
                       cnt);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(range_map::map_equalize_kernel, dim3(p.eq_grid), dim3(p.block), 0, s, x, n, ldx, edges,
                       nbins, (const unsigned long long*)cnt, out, ldo);
    HIP_TRY(hipGetLastError());
    return RANGE_OK;
}

}  // extern "C"
