// Host side of the forward calls: range_forward (result in device memory), range_forward_host (the reference's
// contract: a host array) and range_host_copy.  Both calls are encode -> the one-pass route, or pass 1 keeping its
// logits -> pass 2 from them -> finalize; what they share is written once here.  Part of range_hip.hip's translation unit.
#pragma once

// what a model name stands for in the retrieval (range/range.py:103-109): the temperatures of both
// heads (tau_geo 0: no geographic head) and the blend the kernels apply
struct ModelParams { float tau_sem, tau_geo, beta; };

static int model_params(const range_ctx* c, int32_t model, float beta, ModelParams& m) {
    if (model != RANGE_MODEL_RANGE && model != RANGE_MODEL_RANGE_PLUS)
        return fail(RANGE_ERR_INVALID, "unknown model %d", model);
    m.tau_sem = model == RANGE_MODEL_RANGE ? 15.0f : 12.0f;   // range.py:103, 108
    m.tau_geo = model == RANGE_MODEL_RANGE ? 0.0f : 40.0f;    // range.py:109
    // range_set_temperatures (the reference reads args.temp / args.geo_temp at call time, range.py:215, 234)
    if (c->tau_sem_set > 0.f) m.tau_sem = c->tau_sem_set;
    if (c->tau_geo_set > 0.f && model == RANGE_MODEL_RANGE_PLUS) m.tau_geo = c->tau_geo_set;
    m.beta = model == RANGE_MODEL_RANGE ? 1.0f : beta;
    // (here, not only in pass 2: the one-pass route of up to 32 queries never gets there)
    if (!(m.beta >= 0.f && m.beta <= 1.f)) return fail(RANGE_ERR_INVALID, "beta must be in [0,1]");
    return RANGE_OK;
}

// the head of both forward calls: their pointers, the model's parameters
static int forward_head(const range_ctx* c, const double* lonlat, const double* out, int32_t model, float beta, ModelParams& m) {
    if (!c || !lonlat || !out) return fail(RANGE_ERR_INVALID, "null argument");
    return model_params(c, model, beta, m);
}

// Up to 32 queries: the whole retrieval in ONE pass over the bank (attend_small.h) - every CU
// streams its share of keys, locations and values once and accumulates the un-normalised products
// of both heads; small_finalize_kernel sums the workgroups' partials, normalises, blends and packs.
// e-hat / xq of the B queries are in the context's workspace (range_encode ran on `stream`).
static int forward_small(range_ctx* c, int64_t B, const ModelParams& m, double* out, hipStream_t s) {
    SmallArgs a{};
    int rc = softmax_scales(c, B, m.tau_sem, m.tau_geo, RANGE_MAX_TAU, a.k_sem, a.k_geo);
    if (rc) return rc;
    const SmallPlan p = plan_forward_small(c->n_cu, c->bank.n_rows, B, PLAN_CONSTS);
    HIP_TRY(c->pass.ws_small_o.ensure(p.o_floats));
    HIP_TRY(c->pass.ws_small_z.ensure(p.z_floats));
    a.keys = c->bank.d_keys.p;
    a.xyz4 = c->bank.d_xyz4.p;
    a.values = c->bank.d_values.p;
    a.ehat = c->pass.ws_ehat32.p;
    a.xq = c->pass.ws_xq.p;
    a.osum = c->pass.ws_small_o.p;
    a.zsum = c->pass.ws_small_z.p;
    a.B = B;
    a.n_valid = c->bank.n_rows;
    a.n_blocks = p.n_blocks;
    const bool geo = m.tau_geo > 0.f;
    // [0: with the geographic head, 1: without][0: two query tiles per workgroup, 1: one]
    static void (*const small_kernels[2][2])(SmallArgs) = {{attend_small_kernel<true, 2>, attend_small_kernel<true, 1>},
                                                          {attend_small_kernel<false, 2>, attend_small_kernel<false, 1>}};
    {
        ProfScope ps(c, RANGE_PROF_ATTEND, s);
        if (int lrc = launch(small_kernels[!geo][p.nq == 1], dim3((unsigned)p.n_wg), dim3(256), as_lds_bytes(p.nq), s, a)) return lrc;
    }
    rc = launch(small_finalize_kernel, dim3((unsigned)B, 8), dim3(1024), 0, s, c->pass.ws_small_o.p, c->pass.ws_small_z.p,
                p.n_wg, p.qcap, geo ? 1 : 0, geo ? m.beta : 1.0f, c->pass.ws_ehat64.p, out);
    if (rc) return rc;
    c->pass.last_qtiles = 1;
    c->pass.last_splits = p.n_wg;
    return RANGE_OK;
}

// pass 1 over the workspace's B queries, keeping its logits; *kept: it could keep all of them
static int scan_workspace(range_ctx* c, int64_t B, const ModelParams& m, bool* kept, range_stream_t stream) {
    const int rc = range_scan_stats(c, c->pass.ws_ehat32.p, c->pass.ws_xq.p, B, m.tau_sem, m.tau_geo, c->pass.ws_stats.p, 0,
                                    nullptr, nullptr, /*keep_logits=*/1, stream);
    *kept = c->kept.kept_B == B;
    return rc;
}

// pass 2 of the workspace's queries [p0, p1) into the context's split slabs (`map`; the caller finalizes: sums the
// slabs, packs with e-hat): consumes the logits pass 1 kept (recomputes them if they did not fit in memory)
static int attend_workspace(range_ctx* c, int64_t p0, int64_t p1, const ModelParams& m, bool kept, SlabMap* map,
                            range_stream_t stream) {
    return attend_impl(c, c->pass.ws_ehat32.p + p0 * 256, c->pass.ws_xq.p + p0 * 4, p1 - p0, m.tau_sem, m.tau_geo, m.beta,
                       c->pass.ws_stats.p + p0 * 4, nullptr, map, kept ? p0 : -1, stream);
}

// The two passes of the workspace's B queries in the chunks of `plan` (host_plan.h: plan_forward_chunks), the result
// into `out`.  On the caller's stream: pass 1 of chunk 0 as scan_stats_kernel, then per chunk pass 2 and finalize;
// on the context's auxiliary stream, behind chunk 0's pass 1: pass 1 of chunks 1 .. as the kernel that shares a CU
// with pass 2 (pass1_beside.h), each followed by its merge and an event that pass 2 of the chunk waits for.  The
// caller's stream so waits for every piece of auxiliary work in front of the last chunk's pass 2: what the caller
// enqueues afterwards orders as behind a forward of one stream, and the next call's auxiliary work (behind that
// call's chunk 0) orders behind this call's.  Statistics parts have a region per chunk (chunk i + 1 scans while chunk
// i merges); the slabs are reused chunk after chunk: pass 2 and finalize share a stream.
// *chunked false: chunk 0 could not keep its logits and nothing but its scan was enqueued - the caller runs the
// forward as one launch per pass.
static int forward_chunked(range_ctx* c, int64_t B, const ModelParams& m, const FwdChunkPlan& plan, double* out,
                           range_stream_t stream, bool* chunked) {
    *chunked = false;
    ENTER_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    const size_t n_chunks = plan.tiles.size();
    if (!c->ovl.aux_stream) {
        // (a lower priority than the caller's stream was measured too: no difference, profiles/NOTES.md part S)
        HIP_TRY(hipStreamCreateWithFlags(&c->ovl.aux_stream, hipStreamNonBlocking));
    }
    while (c->ovl.events.size() < n_chunks) {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->ovl.events.push_back(e);
    }
    // the workspaces at their largest before anything is in flight: growing one synchronises the device
    int64_t most_tiles = 0;
    for (int t : plan.tiles) most_tiles = std::max<int64_t>(most_tiles, t);
    HIP_TRY(c->pass.ws_stats_parts.ensure((size_t)plan.p1_splits * B * 4));
    HIP_TRY(c->pass.ws_slabs.ensure((size_t)plan.p2_splits * std::min<int64_t>(B, most_tiles * QTILE) * VAL_DIM));
    const float* ehat = c->pass.ws_ehat32.p;
    const float* xq = c->pass.ws_xq.p;
    float* stats = c->pass.ws_stats.p;
    std::vector<int64_t> cuts{0};
    for (int t : plan.tiles) cuts.push_back(std::min<int64_t>(B, cuts.back() + (int64_t)t * QTILE));
    // chunk 0's pass 1
    if (int rc = scan_stats_impl(c, ehat, xq, cuts[1], m.tau_sem, m.tau_geo, stats, 0, nullptr, nullptr, /*keep_logits=*/1, 0, B,
                                 plan.p1_splits, stream))
        return rc;
    if (c->kept.kept_B != cuts[1]) return RANGE_OK;
    *chunked = true;
    HIP_TRY(hipEventRecord(c->ovl.events[0], s));
    HIP_TRY(hipStreamWaitEvent(c->ovl.aux_stream, c->ovl.events[0], 0));
    // (a call that fails half way still leaves the caller's stream behind the auxiliary work it enqueued)
    size_t recorded = 0;
    auto joined = [&](int rc) {
        (void)hipStreamWaitEvent(s, c->ovl.events[recorded], 0);
        return rc;
    };
    for (size_t i = 1; i < n_chunks; ++i) {
        const int64_t q0 = cuts[i], nq = cuts[i + 1] - q0;
        if (int rc = scan_stats_impl(c, ehat + q0 * KEY_DIM, xq + q0 * 4, nq, m.tau_sem, m.tau_geo, stats + q0 * 4, 0, nullptr, nullptr,
                                     /*keep_logits=*/1, q0, B, plan.p1_splits, (range_stream_t)c->ovl.aux_stream, /*beside=*/true,
                                     (size_t)plan.p1_splits * q0 * 4))
            return joined(rc);
        HIP_TRY(hipEventRecord(c->ovl.events[i], c->ovl.aux_stream));
        recorded = i;
    }
    for (size_t i = 0; i < n_chunks; ++i) {
        const int64_t q0 = cuts[i], nq = cuts[i + 1] - q0;
        if (i > 0) HIP_TRY(hipStreamWaitEvent(s, c->ovl.events[i], 0));
        SlabMap map{};
        if (int rc = attend_impl(c, ehat + q0 * KEY_DIM, xq + q0 * 4, nq, m.tau_sem, m.tau_geo, m.beta, stats + q0 * 4, nullptr, &map, q0,
                                 stream, nullptr, 0, plan.p2_splits))
            return joined(rc);
        HIP_TRY(launch_finalize(c->pass.ws_slabs.p, map, c->pass.ws_ehat64.p + q0 * KEY_DIM, nq, 0, nq, out + q0 * RANGE_OUT_DIM, s));
    }
    // (range_last_attend_geometry: the forward's, not its last chunk's)
    c->pass.last_qtiles = (int)((B + QTILE - 1) / QTILE);
    c->pass.last_splits = plan.p2_splits;
    return RANGE_OK;
}

extern "C" {

int range_forward(range_ctx* c, const double* lonlat, int64_t B, int32_t model, float beta,
                  double* out, range_stream_t stream) {
    ModelParams m;
    if (int rc = forward_head(c, lonlat, out, model, beta, m)) return rc;
    // (the workspace's e-hat is claimed for range_topk_last only by a call that succeeds)
    c->pass.ws_queries = 0;
    if (int rc = encode_to_workspace(c, lonlat, B, nullptr, stream)) return rc;
    if (plan_temperatures(m.tau_sem, m.tau_geo, B, c->sw.small_forward).one_pass) {
        // a handful of queries: one pass over the bank (attend_small.h)
        c->pass.ws_queries = B;
        ENTER_DEVICE(c);
        return forward_small(c, B, m, out, (hipStream_t)stream);
    }
    // single GPU: the finalize kernel sums the split slabs itself (same fixed order as
    // reduce_parts_kernel, so the result is bit-identical to attend + finalize)
    // a batch of several rounds of pass 2 against a bank beyond the stream-K walk, exact w @ V, the constant shift,
    // logits kept: in chunks, pass 1 of the next chunk beside pass 2 (forward_chunked)
    if (c->sw.allow_keep && c->bank.pv_mode == RANGE_PV_EXACT && c->bank.has_bank &&
        plan_temperatures(m.tau_sem, m.tau_geo, B, false).shift == SHIFT_CONSTANT) {
        const FwdChunkPlan plan = plan_forward_chunks(c->n_cu, plan_pass1(c->n_cu, c->bank.n_rows, B, false, 0, PLAN_CONSTS),
                                                      plan_pass2(c->n_cu, c->bank.n_rows, B, c->sw.p2_streamk, PLAN_CONSTS),
                                                      c->sw.fwd_overlap);
        if (plan.tiles.size() >= 2) {
            bool chunked = false;
            if (int rc = forward_chunked(c, B, m, plan, out, stream, &chunked)) return rc;
            if (chunked) {
                c->pass.ws_queries = B;
                return RANGE_OK;
            }
        }
    }
    bool kept = false;
    SlabMap map{};
    if (int rc = scan_workspace(c, B, m, &kept, stream)) return rc;
    if (int rc = attend_workspace(c, 0, B, m, kept, &map, stream)) return rc;
    c->pass.ws_queries = B;
    ENTER_DEVICE(c);
    HIP_TRY(launch_finalize(c->pass.ws_slabs.p, map, c->pass.ws_ehat64.p, B, 0, B, out, (hipStream_t)stream));
    return RANGE_OK;
}

int range_host_copy(range_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c || !dst || !src) return fail(RANGE_ERR_INVALID, "null argument");
    if (!c->host.pool) c->host.pool.reset(new HostCopyPool(HostCopyPool::default_threads()));
    c->host.pool->copy(dst, src, bytes);
    return RANGE_OK;
}

// The reference's contract (range/range.py:240): the result is a host array.  The finalize kernel
// runs per slab of queries; each finished slab is copied to pinned staging memory on a copy stream
// while the next is finalized, and the host threads move it into the caller's array (first-touch
// page faults of a fresh array spread over the threads) while the DMA of the next is in flight.
int range_forward_host(range_ctx* c, const double* lonlat, int64_t B, int32_t model, float beta,
                       double* out_host, range_stream_t stream) {
    ModelParams m;
    if (int rc0 = forward_head(c, lonlat, out_host, model, beta, m)) return rc0;
    if (B <= 0) return fail(RANGE_ERR_INVALID, "B must be > 0");
    ENTER_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    const size_t row_bytes = (size_t)RANGE_OUT_DIM * sizeof(double);
    HIP_TRY(c->host.ws_out64.ensure((size_t)B * RANGE_OUT_DIM));
    if (c->host.h_stage_bytes < (size_t)B * row_bytes) {
        if (c->host.h_stage) (void)hipHostFree(c->host.h_stage);
        c->host.h_stage = nullptr;
        c->host.h_stage_bytes = 0;
        HIP_TRY(hipHostMalloc(&c->host.h_stage, (size_t)B * row_bytes, hipHostMallocDefault));
        c->host.h_stage_bytes = (size_t)B * row_bytes;
    }
    if (!c->host.copy_stream) HIP_TRY(hipStreamCreateWithFlags(&c->host.copy_stream, hipStreamNonBlocking));
    if (!c->host.pool) c->host.pool.reset(new HostCopyPool(HostCopyPool::default_threads()));

    // (the workspace's e-hat is claimed for range_topk_last as soon as the encoder is enqueued)
    c->pass.ws_queries = 0;
    int rc = encode_to_workspace(c, lonlat, B, nullptr, stream);
    if (rc) return rc;
    c->pass.ws_queries = B;
    if (plan_temperatures(m.tau_sem, m.tau_geo, B, c->sw.small_forward).one_pass) {
        // a handful of queries: one pass over the bank, one small copy
        rc = forward_small(c, B, m, c->host.ws_out64.p, s);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(c->host.h_stage, c->host.ws_out64.p, (size_t)B * row_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (int rc2 = check_async_error(c)) return rc2;
        std::memcpy(out_host, c->host.h_stage, (size_t)B * row_bytes);
        return RANGE_OK;
    }
    bool kept = false;
    rc = scan_workspace(c, B, m, &kept, stream);
    if (rc) return rc;

    // Pass 2 runs in a few launches over consecutive query ranges (boundaries on query tiles): the
    // device->host copy and the host fill of a part overlap pass 2 of the next, so only the LAST
    // part's copy and fill are exposed - and the parts SHRINK: the rest, 4 096, 512 queries.  What
    // bounds the end is the copy queue (when each slab's copy was seen, measured):
    // 0.205 ms per 1 000 queries (10 KB each at 52 GB/s) against 1.46 ms of pass 2 per 1 000 queries
    // against range_db_large, so a part up to seven times its successor is drained while the
    // successor computes; with (4 096, 1 024) the last slab was seen 0.35 ms after pass 2 ended, with
    // (4 096, 512) 0.15 ms (two equal halves: 1.4 ms).  Part sizes matter on the GPU side too: the
    // split count of pass 2 is chosen per launch so that its workgroups fill whole rounds of the
    // chip (8 query tiles x 32 bank splits, 64 x 4: exactly one round) - measured for 10 000 queries,
    // medians of 30 calls (the box wanders by +-0.1 ms): (4 096, 512) 19.71 ms,
    // (2 048, 256) 19.70, (3 072, 512) 19.87, (4 096, 1 024) 19.96, (1 792, 256) 19.98.
    std::vector<int64_t> cuts{0, B};
    if (B >= 4096) cuts = host_part_cuts(B, {4096, 512}, QTILE);   // (host_plan.h: rounded up to a tile, clamped, monotonic)
    constexpr int64_t SLAB = 1024;
    struct Slab { int64_t q0, nq; hipEvent_t fin, cop; };
    std::vector<Slab> slabs;
    auto give_back = [&]() { for (auto& sl : slabs) { c->ev_pool.push_back(sl.fin); c->ev_pool.push_back(sl.cop); } };
    hipError_t e = hipSuccess;
    for (size_t part = 0; part + 1 < cuts.size() && e == hipSuccess; ++part) {
        const int64_t p0 = cuts[part], p1 = cuts[part + 1];
        if (p1 <= p0) continue;
        SlabMap map{};
        rc = attend_workspace(c, p0, p1, m, kept, &map, stream);
        if (rc) { (void)hipDeviceSynchronize(); give_back(); return rc; }
        // finalize per slab (the split slabs of this part are overwritten by the next part's pass 2,
        // which is behind these kernels in stream order)
        // (the last part in slabs of 256 queries: its copies and fills are what the caller waits for,
        // and they pipeline per slab)
        const int64_t slab = part + 2 == cuts.size() && cuts.size() > 2 ? SLAB / 4 : SLAB;
        for (int64_t q0 = p0; q0 < p1 && e == hipSuccess; q0 += slab) {
            Slab sl{q0, std::min<int64_t>(slab, p1 - q0), c->get_event(), c->get_event()};
            slabs.push_back(sl);
            e = launch_finalize(c->pass.ws_slabs.p, map, c->pass.ws_ehat64.p + p0 * 256, p1 - p0, q0 - p0, sl.nq,
                                c->host.ws_out64.p + p0 * RANGE_OUT_DIM, s);
            if (e == hipSuccess) e = hipEventRecord(sl.fin, s);
            if (e == hipSuccess) e = hipStreamWaitEvent(c->host.copy_stream, sl.fin, 0);
            if (e == hipSuccess)
                e = hipMemcpyAsync((char*)c->host.h_stage + q0 * row_bytes, c->host.ws_out64.p + q0 * RANGE_OUT_DIM,
                                   (size_t)sl.nq * row_bytes, hipMemcpyDeviceToHost, c->host.copy_stream);
            if (e == hipSuccess) e = hipEventRecord(sl.cop, c->host.copy_stream);
        }
    }
    // Everything is enqueued and this thread would only wait now: the copy threads touch every page of
    // the caller's array meanwhile (one write per 4 KB page; the data follows).  A fresh array is
    // 25 000 untouched pages per 10 000 queries: faulted here, under the GPU's shadow, the fills
    // below are plain copies - also the last part's, which the caller waits for.
    if (e == hipSuccess && (size_t)B * row_bytes >= ((size_t)1 << 20)) {
        char* base = (char*)out_host;
        const size_t bytes = (size_t)B * row_bytes;
        c->host.pool->run([=](int t, int n) {
            const size_t per = ((bytes + n - 1) / n + 4095) & ~(size_t)4095;
            const size_t lo = per * (size_t)t;
            const size_t hi = lo + per < bytes ? lo + per : bytes;
            for (size_t o = lo; o < hi; o += 4096) *(volatile char*)(base + o) = 0;
        });
    }
    for (auto& sl : slabs) {
        if (e != hipSuccess) break;
        e = hipEventSynchronize(sl.cop);
        if (e != hipSuccess) break;
        c->host.pool->copy((char*)out_host + sl.q0 * row_bytes, (const char*)c->host.h_stage + sl.q0 * row_bytes,
                      (size_t)sl.nq * row_bytes);
    }
    if (e != hipSuccess) {
        (void)hipDeviceSynchronize();
        give_back();
        return fail(RANGE_ERR_HIP, "range_forward_host: %s", hipGetErrorString(e));
    }
    give_back();
    return check_async_error(c);
}

}  // extern "C"
