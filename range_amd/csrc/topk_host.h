// Host side of the top-k side channel: range_topk_stream with its two routes (the streaming scan of topk_stream.h, the
// batch-scale route of topk_gemm.h), range_topk_last, the timed variants, range_stream_read_timed and the exact count.
// Part of range_hip.hip's translation unit.
#pragma once

// the counters of range_topk_stream_exact_count: [0] brute-force queries, [1] candidates ranked (diagnostic)
static int ensure_exact_count(range_ctx* c, hipStream_t s) {
    if (c->topk.ws_exact_count.p) return RANGE_OK;
    HIP_TRY(c->topk.ws_exact_count.ensure(2));
    HIP_TRY(hipMemsetAsync(c->topk.ws_exact_count.p, 0, 2 * sizeof(int32_t), s));
    return RANGE_OK;
}

// the batch-scale route of range_topk_stream (topk_gemm.h): group maxima -> per-query threshold ->
// candidates -> float32 re-rank
static int topk_gemm_route(range_ctx* c, const TopkPlan& p, const float* ehat32, int64_t B, int32_t k, float* topk_val,
                           int64_t* topk_idx, int repeats, float* avg_us, hipStream_t s) {
    TopkGemmArgs ga{};
    if (c->bank.tg_key_scale == 0.f) {
        // the fp16 copy of the keys, scaled so that the largest row norm lies in [2^13, 2^14)
        const float ks = (float)std::ldexp(1.0, 14 - p.key_e2);
        const int64_t n_tiles = c->bank.n_pad / BLK;
        HIP_TRY(c->bank.d_keys_f16.ensure((size_t)n_tiles * (TSB_TILE_BYTES / 4)));
        const int64_t threads = n_tiles * 8 * 64;
        int rc = launch(keyfrag_f16_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, c->bank.d_keys.p,
                        c->bank.n_pad, n_tiles, ks, reinterpret_cast<u32x4*>(c->bank.d_keys_f16.p));
        if (rc) return rc;
        c->bank.tg_key_scale = ks;
    }
    ga.keys_f16 = c->bank.d_keys_f16.p;
    ga.keys = c->bank.d_keys.p;
    ga.ehat = ehat32;
    ga.B = B;
    ga.n_valid = c->bank.n_rows;
    ga.n_blocks = p.n_blocks;
    ga.n_qblocks = p.n_qblocks;
    ga.n_splits = p.n_splits;
    ga.k = k;
    ga.row_offset = c->bank.row_offset;
    ga.oval = topk_val;
    ga.oidx = topk_idx;
    if (int rc = ensure_exact_count(c, s)) return rc;
    ga.exact_count = c->topk.ws_exact_count.p;
    HIP_TRY(c->topk.ws_tg_gmax.ensure((size_t)ga.n_splits * 2 * B * 4));
    HIP_TRY(c->topk.ws_tg_theta.ensure((size_t)B * 2));
    HIP_TRY(c->topk.ws_tg_cnt.ensure((size_t)B * ga.n_splits * 4));
    HIP_TRY(c->topk.ws_tg_cand.ensure((size_t)B * ga.n_splits * 4 * TG_CAP_L));
    HIP_TRY(c->topk.ws_tg_ovf.ensure((size_t)B));
    ga.ovf = c->topk.ws_tg_ovf.p;
    HIP_TRY(c->topk.ws_tg_qfrag.ensure((size_t)p.n_groups * 8 * 64 * 4));
    HIP_TRY(c->topk.ws_tg_qscale.ensure((size_t)B));
    ga.qfrag = c->topk.ws_tg_qfrag.p;
    ga.gmax = c->topk.ws_tg_gmax.p;
    ga.theta = c->topk.ws_tg_theta.p;
    ga.cnt = c->topk.ws_tg_cnt.p;
    ga.cand = c->topk.ws_tg_cand.p;
    const dim3 ggrid((unsigned)p.grid), gblock(TG_WAVES * 64);
    return timed_repeat(c, s, repeats, avg_us, [&]() -> int {
        {
            ProfScope ps(c, RANGE_PROF_TOPK_STREAM, s);
            if (int lrc = launch(qfrag_f16_kernel, dim3((unsigned)p.n_groups), dim3(256), 0, s, ehat32, B,
                                 reinterpret_cast<u32x4*>(c->topk.ws_tg_qfrag.p), c->topk.ws_tg_qscale.p))
                return lrc;
            ga.tile_stride = p.tile_stride;
            if (int lrc = launch(topk_gemm_kernel<0>, ggrid, gblock, TG_LDS_BYTES, s, ga)) return lrc;
            ga.tile_stride = 1;
            if (int lrc = launch(topk_gemm_threshold_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, ga.gmax,
                                 ga.n_splits * 2, B, ehat32,
                                 (float)((double)TG_EPS_REL * (double)c->bank.key_norm_max * (double)c->bank.tg_key_scale),
                                 c->bank.key_norm_max > 0.f ? (float)std::log2((double)c->bank.key_norm_max) : -INFINITY,
                                 c->topk.ws_tg_qscale.p, c->topk.ws_tg_theta.p))
                return lrc;
            if (int lrc = launch(topk_gemm_kernel<1>, ggrid, gblock, TG_LDS_BYTES, s, ga)) return lrc;
        }
        ProfScope ps(c, RANGE_PROF_TOPK_MERGE, s);
        if (int lrc = launch(topk_gemm_rerank_kernel, dim3((unsigned)B), dim3(256), 0, s, ga)) return lrc;
        return launch(topk_gemm_brute_kernel, dim3((unsigned)std::min<int64_t>(B, 2 * c->n_cu)), dim3(256), 0, s, ga);
    });
}

// repeats > 1 (range_topk_stream_timed): the whole call's launches are enqueued `repeats` times
// back to back between ONE pair of events (identical launches, identical results) and *avg_us
// receives the time per call.
static int topk_stream_impl(range_ctx* c, const float* ehat32, int64_t B, int32_t k, float* topk_val,
                            int64_t* topk_idx, int repeats, float* avg_us, range_stream_t stream) {
    if (!c || !ehat32 || !topk_val || !topk_idx) return fail(RANGE_ERR_INVALID, "null argument");
    if (!c->bank.has_bank) return fail(RANGE_ERR_STATE, "bank not set (range_set_bank)");
    if (B <= 0 || k <= 0 || k > MAX_TOPK) return fail(RANGE_ERR_INVALID, "bad B or k");
    if (int rc0 = check_async_error(c)) return rc0;
    ENTER_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    const TopkPlan p = plan_topk(c->n_cu, c->bank.n_rows, B, c->bank.key_norm_max, c->sw.topk_gemm, c->sw.topks_bf16,
                                 c->sw.topks_fused, c->sw.topks_force_exact, c->sw.tg_sample, PLAN_CONSTS);
    if (p.gemm) return topk_gemm_route(c, p, ehat32, B, k, topk_val, topk_idx, repeats, avg_us, s);
    HIP_TRY(c->topk.ws_cand_keys.ensure(p.cand_keys));
    HIP_TRY(c->topk.ws_cand_dmax.ensure(p.cand_dmax));
    if (int rc = ensure_exact_count(c, s)) return rc;
    const bool bf16 = c->sw.topks_bf16;
    TopkStreamArgs a{};
    a.keys = c->bank.d_keys.p;
    a.ehat = ehat32;
    a.cand = c->topk.ws_cand_keys.p;
    a.dmax = c->topk.ws_cand_dmax.p;
    a.B = B;
    a.n_valid = c->bank.n_rows;
    a.n_blocks = p.n_blocks;
    a.n_groups = p.n_groups;
    a.keys_bf16 = c->bank.d_keys_bf16.p;
    a.sync = c->topk.ws_topk_sync.p;
    a.err = c->d_async_err ? c->d_async_err + RANGE_ASYNC_WORD_TOPK : nullptr;
    a.fused = p.fused ? 1 : 0;
    a.k = k;
    a.row_offset = c->bank.row_offset;
    a.force_exact = c->sw.topks_force_exact ? 1 : 0;
    a.exact_count = c->topk.ws_exact_count.p;
    a.eps_rel = bf16 ? TSB_EPS_REL : 0.f;
    a.kmax = c->bank.key_norm_max;
    a.oval = topk_val;
    a.oidx = topk_idx;
    constexpr int LIST = 4;                  // depth of the per-lane lists
    constexpr int NWV = 4, DEP = 2;
    // [0: bf16 prefilter, 1: float32 keys][query groups per pass - 1]; all with workgroups of 4 waves
    static void (*const stream_kernels[2][2])(TopkStreamArgs) = {
        {topk_stream_bf16_kernel<1, LIST>, topk_stream_bf16_kernel<2, LIST>},
        {topk_stream_kernel<1, LIST, NWV, DEP>, topk_stream_kernel<2, LIST, NWV, DEP>}};
    return timed_repeat(c, s, repeats, avg_us, [&]() -> int {
        for (int x = 0; x < 8; ++x) a.sync_base[x] = c->topk.topk_sync_base[x];
        a.debug_giveup = p.fused && c->debug_giveup_next ? 1 : 0;
        {
            ProfScope ps(c, RANGE_PROF_TOPK_STREAM, s);
            if (int rc = launch(stream_kernels[!bf16][p.G - 1], dim3((unsigned)p.n_wg), dim3(NWV * 64), TOPKS_LDS_BYTES, s, a))
                return rc;
        }
        if (p.fused) {
            // every workgroup of the launch takes one ticket of its shard (blockIdx % 8)
            for (int x = 0; x < 8; ++x) c->topk.topk_sync_base[x] += (uint32_t)((p.n_wg - x + 7) >> 3);
            c->debug_giveup_next = false;
            return RANGE_OK;
        }
        ProfScope ps(c, RANGE_PROF_TOPK_MERGE, s);
        return launch(topk_merge_kernel<TOPKS_WL>, dim3((unsigned)B), dim3(256), TOPKM_LDS_BYTES, s, a, p.n_wg);
    });
}

extern "C" {

int range_topk_stream(range_ctx* c, const float* ehat32, int64_t B, int32_t k, float* topk_val,
                      int64_t* topk_idx, range_stream_t stream) {
    return topk_stream_impl(c, ehat32, B, k, topk_val, topk_idx, 1, nullptr, stream);
}

// forward(coords, return_topk=k): the top-k of the queries the context's last range_forward /
// range_forward_host call embedded - their e-hat (float32) is still in the workspace, so the side
// channel costs its scan only: no second encoder pass.
int range_topk_last(range_ctx* c, int64_t B, int32_t k, float* topk_val, int64_t* topk_idx,
                    range_stream_t stream) {
    if (!c || !topk_val || !topk_idx) return fail(RANGE_ERR_INVALID, "null argument");
    if (B <= 0 || c->pass.ws_queries != B)
        return fail(RANGE_ERR_STATE, "range_topk_last(B=%lld): the workspace holds the e-hat of %lld queries (the last "
                    "range_forward / range_forward_host call of this context)", (long long)B, (long long)c->pass.ws_queries);
    return topk_stream_impl(c, c->pass.ws_ehat32.p, B, k, topk_val, topk_idx, 1, nullptr, stream);
}

int range_topk_stream_timed(range_ctx* c, const float* ehat32, int64_t B, int32_t k, float* topk_val,
                            int64_t* topk_idx, int32_t repeats, float* avg_us, range_stream_t stream) {
    if (repeats < 2 || !avg_us) return fail(RANGE_ERR_INVALID, "repeats must be >= 2 and avg_us non-null");
    return topk_stream_impl(c, ehat32, B, k, topk_val, topk_idx, repeats, avg_us, stream);
}

// A plain one-launch streaming read of the same bytes the top-k scan streams (`passes` times over
// the bf16 or the float32 copy of the keys): the ceiling a launch of that size can reach on this
// chip, measured the same way as range_topk_stream_timed (stream_read_kernel, topk_stream.h).
int range_stream_read_timed(range_ctx* c, int32_t f32_keys, int32_t passes, int32_t repeats, float* avg_us,
                            range_stream_t stream) {
    if (!c || !avg_us) return fail(RANGE_ERR_INVALID, "null argument");
    if (!c->bank.has_bank) return fail(RANGE_ERR_STATE, "bank not set (range_set_bank)");
    if (passes < 1 || repeats < 2) return fail(RANGE_ERR_INVALID, "passes must be >= 1 and repeats >= 2");
    ENTER_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_tiles = c->bank.n_pad / BLK;
    const u32x4* src = f32_keys ? reinterpret_cast<const u32x4*>(c->bank.d_keys.p) : reinterpret_cast<const u32x4*>(c->bank.d_keys_bf16.p);
    const int64_t n16 = f32_keys ? c->bank.n_pad * (KEY_DIM * 4 / 16) : n_tiles * (TSB_TILE_BYTES / 16);
    const int grid = 4 * c->n_cu;
    HIP_TRY(c->topk.ws_read_sink.ensure((size_t)grid));
    const auto read_once = [&]() -> int {
        return launch(stream_read_kernel, dim3(grid), dim3(256), 0, s, src, n16, passes, c->topk.ws_read_sink.p);
    };
    if (int rc = read_once()) return rc;   // (warm-up)
    return timed_repeat(c, s, repeats, avg_us, read_once);
}

int range_topk_stream_exact_count(range_ctx* c, int64_t* count) {
    if (!c || !count) return fail(RANGE_ERR_INVALID, "null argument");
    *count = 0;
    if (!c->topk.ws_exact_count.p) return RANGE_OK;
    ENTER_DEVICE(c);
    int32_t v = 0;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(&v, c->topk.ws_exact_count.p, sizeof v, hipMemcpyDeviceToHost));
    *count = v;
    return check_async_error(c);     // (a merging workgroup of an earlier fused call that gave up)
}

}  // extern "C"
