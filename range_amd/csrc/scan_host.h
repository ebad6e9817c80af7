// Host side of the two passes over the bank: pass 1 (range_scan_stats, range_scan_stats_at), the statistics from the
// kept logits (range_stats_kept), pass 2 (range_attend, range_attend_kept, range_attend_diag) and the entry points a
// sharded job merges and finalizes with (range_merge_stats, range_merge_topk, range_finalize, range_blend).  Each
// kernel table sits at the launch that indexes it.  Part of range_hip.hip's translation unit.
#pragma once

static_assert(MAX_TAU_CONSTANT == RANGE_MAX_TAU && MAX_TAU_SHARP == RANGE_MAX_TAU_SHARP, "host_plan.h and range_hip.h disagree");

// Preconditions and scales of every kernel that forms softmax weights: k_sem / k_geo are the
// temperatures in the kernels' base-2 form (k_geo 0: no geographic head).  max_tau: the cap that fits
// the caller - RANGE_MAX_TAU for a kernel with the constant shift m = tau * log2(e), RANGE_MAX_TAU_SHARP
// for one that takes its shift from the statistics (pass 2) or keeps a running maximum.
static int softmax_scales(range_ctx* c, int64_t B, float tau_sem, float tau_geo, float max_tau, float& k_sem, float& k_geo) {
    if (!c->bank.has_bank) return fail(RANGE_ERR_STATE, "bank not set (range_set_bank)");
    if (!c->bank.has_values)
        return fail(RANGE_ERR_STATE, "keys-only bank (range_set_keys): only range_topk_stream runs on it");
    if (B <= 0) return fail(RANGE_ERR_INVALID, "B must be > 0");
    if (!plan_temperatures(tau_sem, tau_geo, B, false).valid)
        return fail(RANGE_ERR_INVALID, "temperatures must be finite, > 0 and at most %g (tau_sem %g, tau_geo %g; tau_geo <= 0: "
                    "no geographic head): beyond that the softmax is an argmax to float32 precision",
                    (double)RANGE_MAX_TAU_SHARP, (double)tau_sem, (double)tau_geo);
    // the constant shift m = tau * log2(e) of the softmax statistics needs every logit <= 1:
    // unit keys (range/range.py:85-89).  A bank that skipped that preparation would overflow.
    // (written as !(x <= 1.001): a row holding NaN or infinity makes the largest norm NaN / inf and is
    // refused too - the reference would return NaN for EVERY query of every batch against such a bank,
    // range/range.py:213-215: one NaN logit poisons each softmax row)
    if (!(c->bank.key_norm_max <= 1.001f))
        return fail(RANGE_ERR_INVALID, "bank keys are not L2-normalised or not finite (largest row norm %.4f): the softmax of "
                    "range_scan_stats / range_attend needs unit keys, as range/range.py:85-89 prepares them "
                    "(range_topk_stream accepts any norm)", (double)c->bank.key_norm_max);
    if (tau_geo > 0.f && !(c->bank.xyz_norm_max <= 1.001f))
        return fail(RANGE_ERR_INVALID, "bank locations are not unit vectors or not finite (largest row norm %.4f): the geographic "
                    "softmax needs them as range/utils/utils.py:11-16 computes them", (double)c->bank.xyz_norm_max);
    // a kernel with the constant shift m = tau * log2(e): the smallest term 2^(-2m) must stay a normal float32
    if (tau_sem > max_tau || tau_geo > max_tau)
        return fail(RANGE_ERR_INVALID, "internal: temperatures above %g reached a constant-shift kernel", (double)max_tau);
    const double LOG2E = 1.4426950408889634;
    k_sem = (float)(tau_sem * LOG2E);
    k_geo = tau_geo > 0.f ? (float)(tau_geo * LOG2E) : 0.f;
    return RANGE_OK;
}

// what both passes share of their arguments, into a zeroed `a`; the geometry (n_blocks, n_qtiles,
// n_splits, sk_*) and the outputs are the caller's, from its plan
static int fill_scan_args(range_ctx* c, ScanArgs& a, const float* ehat32, const float* xq, int64_t B,
                          float tau_sem, float tau_geo) {
    if (int rc = softmax_scales(c, B, tau_sem, tau_geo, RANGE_MAX_TAU_SHARP, a.k_sem, a.k_geo)) return rc;
    a.keys = c->bank.d_keys.p;
    a.xyz4 = c->bank.d_xyz4.p;
    a.values = c->bank.d_values.p;
    a.ehat = ehat32;
    a.xq = xq;
    a.B = B;
    a.n_valid = c->bank.n_rows;
    a.beta = 1.f;
    a.sk_cols = 1;
    return RANGE_OK;
}

// the merge of the statistics' n_parts parts for B queries: a merging workgroup takes one query per wave (4), or
// one per thread (256)
static int launch_merge_stats(bool by_wave, const float* parts, int32_t n_parts, int64_t B, float* out, hipStream_t s) {
    const int per_wg = by_wave ? 4 : 256;
    return launch(by_wave ? merge_stats_wave_kernel : merge_stats_kernel, dim3((unsigned)((B + per_wg - 1) / per_wg)), dim3(256),
                  0, s, parts, n_parts, B, out);
}

// finalize_kernel for queries [q0, q0 + nq) of the B that `slabs` / `map`, `ehat64` and `out` hold: sums the split
// slabs (the fixed order of reduce_parts_kernel) and packs the result with e-hat.  Returns the launch's HIP status
// (range_forward_host keeps several of them in flight).
static hipError_t launch_finalize(const float* slabs, const SlabMap& map, const double* ehat64, int64_t B, int64_t q0,
                                  int64_t nq, double* out, hipStream_t s) {
    const int64_t n = nq * 320;
    hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, slabs, map, ehat64, B, q0, nq, out);
    return hipGetLastError();
}

// first_query / total_queries / force_splits: range_scan_stats_at (a scan in chunks whose
// kept logits share one workspace); a plain range_scan_stats is the chunk [0, B) of a scan of B.
// beside / parts_offset (range_forward's later chunks, on a stream of their own): the persistent kernel that fits
// next to pass 2 (pass1_beside.h), its statistics parts `parts_offset` floats into the workspace - a region of
// the chunk's own, since the chunk before it may still be merging.
static int scan_stats_impl(range_ctx* c, const float* ehat32, const float* xq32, int64_t B, float tau_sem,
                           float tau_geo, float* stats, int topk, float* topk_val, int64_t* topk_idx,
                           int32_t keep_logits, int64_t first_query, int64_t total_queries, int32_t force_splits,
                           range_stream_t stream, bool beside = false, size_t parts_offset = 0) {
    if (!c || !ehat32 || !xq32 || !stats) return fail(RANGE_ERR_INVALID, "null argument");
    if (topk < 0 || topk > MAX_TOPK) return fail(RANGE_ERR_INVALID, "topk must be in [0,%d]", MAX_TOPK);
    if (topk > 0 && (!topk_val || !topk_idx)) return fail(RANGE_ERR_INVALID, "topk outputs null");
    if (first_query < 0 || first_query % QTILE != 0)
        return fail(RANGE_ERR_INVALID, "first_query must be a non-negative multiple of %d", QTILE);
    if (B > 0 && first_query + B > total_queries)
        return fail(RANGE_ERR_INVALID, "queries [%lld, %lld) exceed the scan's %lld", (long long)first_query,
                    (long long)(first_query + B), (long long)total_queries);
    if (force_splits < 0) return fail(RANGE_ERR_INVALID, "n_splits must be >= 0");
    ENTER_DEVICE(c);
    ScanArgs a{};
    hipStream_t s = (hipStream_t)stream;
    // a later chunk extends the scan only in order, and only when the first chunk could keep
    const bool extends = first_query > 0 && c->kept.kept_B == first_query && c->kept.kept_total == total_queries;
    if (first_query > 0 && !extends) keep_logits = 0;
    if (!extends) c->kept.kept_B = 0;
    // The logits of this call are written to HBM when the caller asks for them (plain scan) or
    // when a larger batch wants its top-k: pass 1 then runs WITHOUT the in-loop list maintenance
    // (which costs more than its MFMAs) and a streaming selection over the kept logits follows.
    // 4 B per (query, bank row) of this context's shard; not done when that would take more than
    // half of the free device memory (pass 2 then recomputes, top-k uses the in-scan lists).
    // A top-k batch always selects from the kept logits: measured (tools/topk_total_time.py), the
    // selection wins at every batch size, so the in-scan lists (scan_stats_kernel<.., true>) only
    // serve contexts that cannot keep logits.
    bool write_logits = c->sw.allow_keep && (topk > 0 ? B > 0 : keep_logits != 0);
    const int64_t n_qtiles = (total_queries + QTILE - 1) / QTILE, n_blocks = (c->bank.n_rows + BLK - 1) / BLK;
    const size_t need = (size_t)n_qtiles * n_blocks * 1024;
    if (write_logits && extends) {
        // (the workspace was sized for the whole scan by its first chunk)
        if (need > c->kept.ws_logits.n || c->kept.kept_blocks != n_blocks) { write_logits = false; c->kept.kept_B = 0; }
    } else if (write_logits && need > c->kept.ws_logits.n) {        // (hipMemGetInfo is slow: only when growing)
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        if (need * sizeof(float) <= free_b / 2) {
            HIP_TRY(c->kept.ws_logits.ensure(need));
        } else {
            write_logits = false;
            if (!c->kept.warned_no_keep) {   // once per context: pass 2 will recompute the logits (25 % more MFMAs)
                c->kept.warned_no_keep = true;
                std::fprintf(stderr, "librange_hip: the logits of %lld queries x %lld bank rows (%.1f GB) do not fit in "
                             "half of the free device memory (%.1f GB free): not kept, pass 2 recomputes them\n",
                             (long long)B, (long long)c->bank.n_rows, need * 4e-9, free_b * 1e-9);
            }
        }
    }
    const bool topk_from_kept = topk > 0 && write_logits;
    const bool topk_scan = topk > 0 && !topk_from_kept;
    int rc = fill_scan_args(c, a, ehat32, xq32, B, tau_sem, tau_geo);
    if (rc) return rc;
    // temperatures above RANGE_MAX_TAU: the running-max form of pass 1 (pass1_sharp.h), for both heads
    const TempRoute route = plan_temperatures(tau_sem, tau_geo, B, c->sw.small_forward);
    if (topk_scan && !route.topk_scan_ok)
        return fail(RANGE_ERR_INVALID, "range_scan_stats(topk > 0) at a temperature above %g needs to keep its logits (this "
                    "context cannot: RANGE_KEEP_LOGITS=0 or not enough free memory): take the top-k from range_topk_stream",
                    (double)RANGE_MAX_TAU);
    const Pass1Plan p = plan_pass1(c->n_cu, c->bank.n_rows, B, topk_scan, force_splits, PLAN_CONSTS);
    a.n_blocks = p.n_blocks;
    a.n_qtiles = p.n_qtiles;
    a.n_splits = p.n_splits;
    if (write_logits) a.logits = c->kept.ws_logits.p;
    a.qt_offset = (int32_t)(first_query / QTILE);
    if (topk_from_kept) {
        HIP_TRY(c->kept.ws_rowmax.ensure(p.part_floats));
        HIP_TRY(c->kept.ws_theta.ensure((size_t)B));
        a.rowmax = c->kept.ws_rowmax.p;
    }
    HIP_TRY(c->pass.ws_stats_parts.ensure(parts_offset + p.part_floats));
    a.out = c->pass.ws_stats_parts.p + parts_offset;
    if (topk_scan) {
        HIP_TRY(c->topk.ws_cand_val.ensure(p.part_floats * MAX_TOPK));
        HIP_TRY(c->topk.ws_cand_idx.ensure(p.part_floats * MAX_TOPK));
        a.cand_val = c->topk.ws_cand_val.p;
        a.cand_idx = c->topk.ws_cand_idx.p;
    }
    const bool geo = tau_geo > 0.f;
    // [0: with the geographic head, 1: without][0: with in-scan top-k lists, 1: without]
    static void (*const scan_kernels[2][2])(ScanArgs) = {{scan_stats_kernel<true, true>, scan_stats_kernel<true, false>},
                                                        {scan_stats_kernel<false, true>, scan_stats_kernel<false, false>}};
    // pass 1 with a running maximum (pass1_sharp.h) [0: with the geographic head, 1: without]
    static void (*const sharp_kernels[2])(ScanArgs) = {sharp_scan_stats_kernel<true>, sharp_scan_stats_kernel<false>};
    // pass 1 beside pass 2 (pass1_beside.h): one persistent workgroup per CU [0: with the geographic head, 1: without]
    static void (*const beside_kernels[2])(ScanArgs) = {scan_stats_beside_kernel<true>, scan_stats_beside_kernel<false>};
    if (beside && (topk > 0 || route.shift == SHIFT_RUNNING_MAX))
        return fail(RANGE_ERR_INVALID, "internal: pass 1 beside pass 2 has the constant shift and no top-k");
    {
        ProfScope ps(c, RANGE_PROF_SCAN_STATS, s);
        if (beside) {
            if (int lrc = launch(beside_kernels[!geo], dim3((unsigned)std::min(c->n_cu, p.grid)), dim3(256), BESIDE_LDS_BYTES, s, a)) return lrc;
        } else {
            void (*const kernel)(ScanArgs) = route.shift == SHIFT_RUNNING_MAX ? sharp_kernels[!geo] : scan_kernels[!geo][!topk_scan];
            if (int lrc = launch(kernel, dim3((unsigned)p.grid), dim3(256), SCAN_LDS_BYTES, s, a)) return lrc;
        }
    }
    if (a.logits && keep_logits) {
        c->kept.kept_B = first_query + B;
        c->kept.kept_total = total_queries;
        c->kept.kept_blocks = a.n_blocks;
    }
    rc = launch_merge_stats(p.merge_by_wave, a.out, a.n_splits, B, stats, s);
    if (rc) return rc;
    int n_parts = a.n_splits, per_part = 4 * MAX_TOPK;     // the in-scan lists
    if (topk_from_kept) {
        const int n_chunks = p.topk_chunks;
        HIP_TRY(c->topk.ws_cand_val.ensure((size_t)n_chunks * B * MAX_TOPK));
        HIP_TRY(c->topk.ws_cand_idx.ensure((size_t)n_chunks * B * MAX_TOPK));
        rc = launch(topk_threshold_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s,
                    c->kept.ws_rowmax.p, a.n_splits, B, c->kept.ws_theta.p);
        if (rc) return rc;
        rc = launch(topk_from_logits_kernel, dim3((unsigned)((p.topk_slots + 3) / 4), (unsigned)n_chunks),
                    dim3(256), 0, s, c->kept.ws_logits.p, a.n_blocks, B, c->bank.n_rows, n_chunks,
                    c->kept.ws_theta.p, c->topk.ws_cand_val.p, c->topk.ws_cand_idx.p);
        if (rc) return rc;
        n_parts = n_chunks;
        per_part = MAX_TOPK;
    }
    if (topk <= 0) return RANGE_OK;
    return launch(merge_topk_wave_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, c->topk.ws_cand_val.p,
                  c->topk.ws_cand_idx.p, n_parts, B, per_part, topk, c->bank.row_offset, topk_val, topk_idx);
}

// pass 2 into the context's split slabs; when `partial` is non-null the slabs are then summed
// (fixed order) into it, otherwise the caller consumes the slabs (n_splits_out of them) itself.
// kept_first >= 0: queries [kept_first, kept_first + B) of the last scan whose logits were kept
// (attend_stored_kernel; ehat32 is not read); kept_first < 0: recompute the logits.
// diag_dev non-null (range_attend_diag): the instrumented build of the recomputing kernel, always in
// the split scheme, with the slabs as its only output.  force_splits > 0: the split scheme's split count
// (range_forward's chunks take the whole batch's).
static int attend_impl(range_ctx* c, const float* ehat32, const float* xq32, int64_t B, float tau_sem,
                       float tau_geo, float beta, const float* stats_global, float* partial,
                       SlabMap* map_out, int64_t kept_first, range_stream_t stream,
                       unsigned long long* diag_dev = nullptr, int64_t diag_capacity = 0, int32_t force_splits = 0) {
    if (!c || (!ehat32 && kept_first < 0) || !xq32 || !stats_global)
        return fail(RANGE_ERR_INVALID, "null argument");
    if (kept_first >= 0) {
        if (c->kept.kept_B <= 0) return fail(RANGE_ERR_STATE, "no kept logits (range_scan_stats with keep_logits)");
        if (kept_first % QTILE != 0) return fail(RANGE_ERR_INVALID, "first kept query must be a multiple of %d", QTILE);
        if (kept_first + B > c->kept.kept_B)
            return fail(RANGE_ERR_INVALID, "queries [%lld, %lld) exceed the %lld kept", (long long)kept_first,
                        (long long)(kept_first + B), (long long)c->kept.kept_B);
    }
    if (!diag_dev && !(beta >= 0.f && beta <= 1.f)) return fail(RANGE_ERR_INVALID, "beta must be in [0,1]");
    ENTER_DEVICE(c);
    ScanArgs a{};
    int rc = fill_scan_args(c, a, ehat32, xq32, B, tau_sem, tau_geo);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const bool geo = tau_geo > 0.f;
    const bool bf16x3 = kept_first >= 0 && c->bank.pv_mode == RANGE_PV_BF16X3;
    if (bf16x3 && plan_temperatures(tau_sem, tau_geo, B, false).shift == SHIFT_RUNNING_MAX)
        return fail(RANGE_ERR_INVALID, "pv mode bf16x3 is not supported at temperatures above %g", (double)RANGE_MAX_TAU);
    // (stream-K: the exact kernels only)
    const Pass2Plan p = plan_pass2(c->n_cu, c->bank.n_rows, B, c->sw.p2_streamk && !bf16x3 && !diag_dev, PLAN_CONSTS, force_splits);
    a.n_blocks = p.n_blocks;
    a.n_qtiles = p.n_qtiles;
    a.n_splits = p.n_splits;
    a.sk_cols = p.sk_cols;
    a.sk_groups = p.sk_groups;
    c->pass.last_qtiles = p.n_qtiles;
    c->pass.last_splits = p.streamk ? p.sk_groups : p.n_splits;
    if (diag_dev) {
        if (!geo) return fail(RANGE_ERR_INVALID, "diagnostic build exists for the geo variant only");
        if ((int64_t)p.grid * 4 * 16 > diag_capacity) return fail(RANGE_ERR_INVALID, "diag buffer too small");
    }
    HIP_TRY(c->pass.ws_slabs.ensure(p.slab_floats));
    const SlabMap map{a.n_splits, a.sk_groups, a.n_blocks, a.n_qtiles, a.sk_cols};
    a.out = c->pass.ws_slabs.p;
    a.stats = stats_global;
    a.beta = geo ? beta : 1.f;
    const dim3 grid((unsigned)p.grid), block(256);
    // [0: with the geographic head, 1: without]
    static void (*const bf16x3_kernels[2])(ScanArgs, const char*, int32_t) = {attend_bf16x3_kernel<true>,
                                                                             attend_bf16x3_kernel<false>};
    static void (*const stored_kernels[2])(ScanArgs) = {attend_stored_kernel<true>, attend_stored_kernel<false>};
    static void (*const recompute_kernels[2])(ScanArgs) = {attend_kernel<true>, attend_kernel<false>};
    if (diag_dev) {
        a.diag = diag_dev;
        return launch(attend_kernel<true, true>, grid, block, ATTEND_LDS_BYTES, s, a);
    }
    if (kept_first >= 0) {
        if (a.n_blocks != c->kept.kept_blocks) return fail(RANGE_ERR_STATE, "bank changed since the logits were kept");
        a.logits = c->kept.ws_logits.p;
        a.qt_offset = (int32_t)(kept_first / QTILE);
        ProfScope ps(c, RANGE_PROF_ATTEND, s);
        if (bf16x3) {
            // opt-in: w @ V on three bf16 planes of both operands (attend_bf16x3.h)
            const int32_t n_groups = (a.n_blocks + 1) / 2;
            if (c->bank.vplanes_groups != n_groups) return fail(RANGE_ERR_STATE, "bf16 planes of the values are missing");
            const char* planes = reinterpret_cast<const char*>(c->bank.d_vplanes.p);
            rc = launch(bf16x3_kernels[!geo], grid, block, PVB2_LDS_BYTES, s, a, planes, n_groups);
        } else {
            rc = launch(stored_kernels[!geo], grid, block, ATTEND_STORED_LDS_BYTES, s, a);
        }
    } else {
        ProfScope ps(c, RANGE_PROF_ATTEND, s);
        rc = launch(recompute_kernels[!geo], grid, block, ATTEND_LDS_BYTES, s, a);
    }
    if (rc) return rc;
    if (map_out) *map_out = map;
    if (partial) {
        const int64_t total4 = B * (VAL_DIM / 4);
        return launch(reduce_parts_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, s,
                      c->pass.ws_slabs.p, map, B, partial);
    }
    return RANGE_OK;
}

extern "C" {

int range_scan_stats(range_ctx* c, const float* ehat32, const float* xq32, int64_t B, float tau_sem,
                     float tau_geo, float* stats, int topk, float* topk_val, int64_t* topk_idx,
                     int32_t keep_logits, range_stream_t stream) {
    return scan_stats_impl(c, ehat32, xq32, B, tau_sem, tau_geo, stats, topk, topk_val, topk_idx, keep_logits,
                           0, B, 0, stream);
}

int range_scan_stats_at(range_ctx* c, const float* ehat32, const float* xq32, int64_t B, float tau_sem,
                        float tau_geo, float* stats, int64_t first_query, int64_t total_queries,
                        int32_t n_splits, range_stream_t stream) {
    return scan_stats_impl(c, ehat32, xq32, B, tau_sem, tau_geo, stats, 0, nullptr, nullptr, /*keep_logits=*/1,
                           first_query, total_queries, n_splits, stream);
}

// the bank splits a pass-1 launch of B queries chooses (no top-k)
int32_t range_p1_splits(const range_ctx* c, int64_t B) {
    if (!c || !c->bank.has_bank || B <= 0) return 0;
    return plan_pass1(c->n_cu, c->bank.n_rows, B, false, 0, PLAN_CONSTS).n_splits;
}

int64_t range_kept_queries(const range_ctx* c) { return c ? c->kept.kept_B : 0; }

int range_stats_kept(range_ctx* c, int64_t first_query, const float* xq32, int64_t B, int32_t n_taus,
                     const float* taus_sem, const float* taus_geo, int32_t n_splits, float* stats,
                     range_stream_t stream) {
    if (!c || !xq32 || !taus_sem || !taus_geo || !stats) return fail(RANGE_ERR_INVALID, "null argument");
    if (n_taus < 1) return fail(RANGE_ERR_INVALID, "n_taus must be >= 1");
    if (n_splits < 0) return fail(RANGE_ERR_INVALID, "n_splits must be >= 0");
    if (c->kept.kept_B <= 0) return fail(RANGE_ERR_STATE, "no kept logits (range_scan_stats with keep_logits)");
    if (first_query < 0 || first_query % QTILE != 0)
        return fail(RANGE_ERR_INVALID, "first kept query must be a non-negative multiple of %d", QTILE);
    if (B <= 0) return fail(RANGE_ERR_INVALID, "B must be > 0");
    if (first_query + B > c->kept.kept_B)
        return fail(RANGE_ERR_INVALID, "queries [%lld, %lld) exceed the %lld kept", (long long)first_query,
                    (long long)(first_query + B), (long long)c->kept.kept_B);
    ENTER_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    const KeptStatsPlan p = plan_kept_stats(c->n_cu, c->bank.n_rows, B, n_taus, n_splits, KEPT_MAX_PAIRS, PLAN_CONSTS);
    KeptStatsArgs a{};
    // every pair: the checks and scales of range_scan_stats (bank, temperatures, norms)
    std::vector<float> k_sem((size_t)n_taus), k_geo((size_t)n_taus);
    for (int i = 0; i < n_taus; ++i)
        if (int rc = softmax_scales(c, B, taus_sem[i], taus_geo[i], RANGE_MAX_TAU_SHARP, k_sem[i], k_geo[i])) return rc;
    if (p.n_blocks != c->kept.kept_blocks) return fail(RANGE_ERR_STATE, "bank changed since the logits were kept");
    HIP_TRY(c->kept.ws_stat_parts.ensure(p.ws_floats));
    a.logits = c->kept.ws_logits.p;
    a.xyz4 = c->bank.d_xyz4.p;
    a.xq = xq32;
    a.out = c->kept.ws_stat_parts.p;
    a.B = B;
    a.n_valid = c->bank.n_rows;
    a.n_blocks = p.n_blocks;
    a.n_qtiles = p.n_qtiles;
    a.n_splits = p.n_splits;
    a.qt_offset = (int32_t)(first_query / QTILE);
    // the statistics from the kept logits (pass1_kept.h) [pairs of the launch - 1][0: some pair has a geographic head, 1: none]
    static void (*const kept_kernels[KEPT_MAX_PAIRS][2])(KeptStatsArgs) = {
        {kept_stats_kernel<1, true>, kept_stats_kernel<1, false>}, {kept_stats_kernel<2, true>, kept_stats_kernel<2, false>},
        {kept_stats_kernel<3, true>, kept_stats_kernel<3, false>}, {kept_stats_kernel<4, true>, kept_stats_kernel<4, false>},
        {kept_stats_kernel<5, true>, kept_stats_kernel<5, false>}, {kept_stats_kernel<6, true>, kept_stats_kernel<6, false>},
        {kept_stats_kernel<7, true>, kept_stats_kernel<7, false>}, {kept_stats_kernel<8, true>, kept_stats_kernel<8, false>}};
    for (const KeptStatsPlan::Group& grp : p.groups) {
        a.sharp_mask = a.geo_mask = 0u;
        for (int i = 0; i < grp.count; ++i) {
            const float ts = taus_sem[grp.first + i], tg = taus_geo[grp.first + i];
            a.k_sem[i] = k_sem[grp.first + i];
            a.k_geo[i] = k_geo[grp.first + i];
            if (kept_pair_shift(ts, tg) == SHIFT_RUNNING_MAX) a.sharp_mask |= 1u << i;
            if (tg > 0.f) a.geo_mask |= 1u << i;
        }
        {
            ProfScope ps(c, RANGE_PROF_KEPT_STATS, s);
            if (int rc = launch(kept_kernels[grp.count - 1][a.geo_mask == 0u], dim3((unsigned)p.grid), dim3(256), 0, s, a)) return rc;
        }
        for (int i = 0; i < grp.count; ++i)
            if (int rc = launch_merge_stats(p.merge_by_wave, c->kept.ws_stat_parts.p + (size_t)i * p.part_floats, p.n_splits, B,
                                            stats + (size_t)(grp.first + i) * B * 4, s))
                return rc;
    }
    return RANGE_OK;
}

int range_attend(range_ctx* c, const float* ehat32, const float* xq32, int64_t B, float tau_sem,
                 float tau_geo, float beta, const float* stats_global, float* partial,
                 range_stream_t stream) {
    if (!partial) return fail(RANGE_ERR_INVALID, "null argument");
    return attend_impl(c, ehat32, xq32, B, tau_sem, tau_geo, beta, stats_global, partial, nullptr, -1, stream);
}

int range_attend_kept(range_ctx* c, int64_t first_query, const float* xq32, int64_t B, float tau_sem,
                      float tau_geo, float beta, const float* stats_global, float* partial,
                      range_stream_t stream) {
    if (!partial) return fail(RANGE_ERR_INVALID, "null argument");
    if (first_query < 0) return fail(RANGE_ERR_INVALID, "first_query must be >= 0");
    return attend_impl(c, nullptr, xq32, B, tau_sem, tau_geo, beta, stats_global, partial, nullptr,
                       first_query, stream);
}

// Diagnostic (not part of the product path): same launch as range_attend with the instrumented
// kernel build; diag_dev receives 16 x uint64 per (workgroup, wave): cycles parked in vmcnt waits,
// barriers, and spent in the PV / QK phases.  Outputs go to the split slabs only.
int range_attend_diag(range_ctx* c, const float* ehat32, const float* xq32, int64_t B, float tau_sem,
                      float tau_geo, float beta, const float* stats_global,
                      unsigned long long* diag_dev, int64_t diag_capacity, range_stream_t stream) {
    if (!c || !ehat32 || !xq32 || !stats_global || !diag_dev) return fail(RANGE_ERR_INVALID, "null argument");
    return attend_impl(c, ehat32, xq32, B, tau_sem, tau_geo, beta, stats_global, nullptr, nullptr, -1, stream,
                       diag_dev, diag_capacity);
}

int range_last_attend_geometry(const range_ctx* c, int32_t* n_query_tiles, int32_t* n_splits) {
    if (!c) return fail(RANGE_ERR_INVALID, "null argument");
    if (n_query_tiles) *n_query_tiles = c->pass.last_qtiles;
    if (n_splits) *n_splits = c->pass.last_splits;
    return RANGE_OK;
}

int range_merge_stats(range_ctx* c, const float* parts, int32_t n_parts, int64_t B, float* out,
                      range_stream_t stream) {
    if (!c || !parts || !out) return fail(RANGE_ERR_INVALID, "null argument");
    if (n_parts <= 0 || B <= 0) return fail(RANGE_ERR_INVALID, "n_parts and B must be > 0");
    ENTER_DEVICE(c);
    return launch_merge_stats(false, parts, n_parts, B, out, (hipStream_t)stream);
}

int range_merge_topk(range_ctx* c, const float* val_parts, const int64_t* idx_parts, int32_t n_parts,
                     int64_t B, int32_t k, float* val_out, int64_t* idx_out, range_stream_t stream) {
    if (!c || !val_parts || !idx_parts || !val_out || !idx_out) return fail(RANGE_ERR_INVALID, "null argument");
    if (n_parts <= 0 || B <= 0 || k <= 0 || k > MAX_TOPK) return fail(RANGE_ERR_INVALID, "bad n_parts/B/k");
    ENTER_DEVICE(c);
    return launch(merge_topk_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0,
                       (hipStream_t)stream, val_parts, (const int32_t*)nullptr, idx_parts, n_parts, B,
                       k, k, (int64_t)0, val_out, idx_out);
}

int range_finalize(range_ctx* c, const float* partials, int32_t n_parts, const double* ehat64,
                   int64_t B, double* out, range_stream_t stream) {
    if (!c || !partials || !ehat64 || !out) return fail(RANGE_ERR_INVALID, "null argument");
    if (n_parts <= 0 || B <= 0) return fail(RANGE_ERR_INVALID, "n_parts and B must be > 0");
    ENTER_DEVICE(c);
    HIP_TRY(launch_finalize(partials, SlabMap{n_parts, 0, 0, 0, 1}, ehat64, B, 0, B, out, (hipStream_t)stream));
    return RANGE_OK;
}

int range_blend(range_ctx* c, const float* G, const float* H, float beta, int64_t B, float* out,
                range_stream_t stream) {
    if (!c || !G || !H || !out) return fail(RANGE_ERR_INVALID, "null argument");
    if (B <= 0) return fail(RANGE_ERR_INVALID, "B must be > 0");
    ENTER_DEVICE(c);
    const int64_t n4 = B * (VAL_DIM / 4);
    return launch(blend_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, G, H, beta, n4, out);
}

}  // extern "C"
