// Host side of the checkerboard task's nearest-support scan (checker_kernel.h).
// Part of range_hip.hip's translation unit, behind engine_ctx.h.
#pragma once

extern "C" {

int range_nearest_support(range_ctx* c, const double* q, int64_t Q, const double* sup, int64_t S, int32_t exclude_self,
                          int32_t max_chunks, int64_t* idx, double* dist, range_stream_t stream) {
    if (!c || !q || !sup || !idx) return fail(RANGE_ERR_INVALID, "null argument");
    if (Q < 1 || S < 1) return fail(RANGE_ERR_INVALID, "Q and S must be > 0");
    if (max_chunks < 0) return fail(RANGE_ERR_INVALID, "max_chunks must be >= 0");
    if (exclude_self && (Q != S || S < 2))
        return fail(RANGE_ERR_INVALID, "exclude_self needs the same Q = S >= 2 points on both sides (Q = %lld, S = %lld)",
                    (long long)Q, (long long)S);
    if (!aligned(q, 8) || !aligned(sup, 8) || !aligned(idx, 8) || !aligned(dist, 8))
        return fail(RANGE_ERR_INVALID, "the device pointers must be 8-byte aligned");
    const CheckerPlan p = checker_plan(Q, S, exclude_self != 0, max_chunks);
    if (!p.valid) return fail(RANGE_ERR_INVALID, "Q = %lld, S = %lld: too many points", (long long)Q, (long long)S);
    ENTER_DEVICE(c);
    const hipStream_t s = (hipStream_t)stream;
    CheckerArgs a{};
    a.q = q;
    a.s = sup;
    a.Q = Q;
    a.S = S;
    a.q_blocks = p.q_blocks;
    a.s_tiles = p.s_tiles;
    a.exclude_self = exclude_self != 0;
    a.idx = idx;
    a.dist = dist;
    if (p.chunks > 1) {
        if (c->checker.ws_a.ensure(p.ws_pairs) != hipSuccess || c->checker.ws_idx.ensure(p.ws_pairs) != hipSuccess)
            return fail(RANGE_ERR_NOMEM, "out of device memory (%zu bytes of partial results)", p.ws_bytes);
        a.part_a = c->checker.ws_a.p;
        a.part_idx = c->checker.ws_idx.p;
    }
    if (int rc = launch(checker_scan_kernel, dim3(p.grid_x, (unsigned)p.chunks), dim3(p.block), p.lds_bytes, s, a)) return rc;
    if (p.chunks == 1) return RANGE_OK;
    return launch(checker_merge_kernel, dim3(p.merge_grid), dim3(p.block), 0, s, (const double*)a.part_a,
                  (const int64_t*)a.part_idx, (int32_t)p.chunks, Q, idx, dist);
}

}  // extern "C"
