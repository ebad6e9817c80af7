// The engine's context and what every launch site shares: the switches, range_ctx, the profiling scope, the one
// launch helper, timed repetition, the plans' constants, the async-error check.  Part of range_hip.hip's
// translation unit, in front of the *_host.h parts.
#pragma once

// the switches of tools/README.md, read from the environment when a context is created; they select
// reference paths for the tests and A/B measurements, the defaults are the product's
struct Switches {
    bool allow_keep = true;          // RANGE_KEEP_LOGITS=0: never keep pass 1's logits (pass 2 recomputes)
    bool enc_split = true;           // RANGE_ENC_SPLIT=0: small batches use the one-kernel encoder too
    bool enc_fused = true;           // RANGE_ENC_FUSED=0: up to 16 queries take the separate small-batch kernels
    bool topks_force_exact = false;  // RANGE_TOPKS_FORCE_EXACT=1: tests of the fallback
    bool topks_bf16 = true;          // RANGE_TOPKS_KEYS=f32: stream the float32 keys (no prefilter)
    bool topks_fused = true;         // RANGE_TOPKS_FUSED=0: the merge as a second launch at every batch size (A/B)
    bool small_forward = true;       // RANGE_SMALL_FORWARD=0: batches of <= 32 queries take the two-pass kernels too (A/B)
    bool topk_gemm = true;           // RANGE_TOPK_GEMM=0: batches beyond 256 queries through the streaming scan too (A/B)
    int tg_sample = TG_SAMPLE;       // RANGE_TG_SAMPLE=n: pass A of the batch top-k looks at every n-th tile (tuning)
    bool p2_streamk = true;          // RANGE_P2_STREAMK=0: pass 2 as one workgroup per (bank split, query tile) (A/B)
    // RANGE_FWD_OVERLAP: range_forward in chunks of query tiles, pass 1 of the next chunk beside pass 2 (host_plan.h:
    // plan_forward_chunks).  Unset (-1): the plan's rule; 0: never (A/B, the tests' yardstick); n > 0: chunks of n
    // query tiles whatever the rule says (tests of the path at small sizes)
    int fwd_overlap = -1;
};

static Switches parse_switches() {
    Switches sw;
    if (const char* e = std::getenv("RANGE_KEEP_LOGITS")) sw.allow_keep = e[0] != '0';
    if (const char* e = std::getenv("RANGE_ENC_SPLIT")) sw.enc_split = e[0] != '0';
    if (const char* e = std::getenv("RANGE_ENC_FUSED")) sw.enc_fused = e[0] != '0';
    if (const char* e = std::getenv("RANGE_TOPKS_FORCE_EXACT")) sw.topks_force_exact = e[0] == '1';
    if (const char* e = std::getenv("RANGE_TOPKS_KEYS")) sw.topks_bf16 = std::strcmp(e, "f32") != 0;
    if (const char* e = std::getenv("RANGE_TOPKS_FUSED")) sw.topks_fused = e[0] != '0';
    if (const char* e = std::getenv("RANGE_SMALL_FORWARD")) sw.small_forward = e[0] != '0';
    if (const char* e = std::getenv("RANGE_TOPK_GEMM")) sw.topk_gemm = e[0] != '0';
    if (const char* e = std::getenv("RANGE_TG_SAMPLE")) sw.tg_sample = std::max(1, std::min(16, std::atoi(e)));
    if (const char* e = std::getenv("RANGE_P2_STREAMK")) sw.p2_streamk = e[0] != '0';
    if (const char* e = std::getenv("RANGE_FWD_OVERLAP")) sw.fwd_overlap = std::max(0, std::atoi(e));
    return sw;
}

struct range_ctx {
    int device = 0;
    int n_cu = 256;
    // (enc_fused / topks_fused are also cleared by check_async_error after a persistent launch gave up)
    Switches sw;
    struct Encoder {
        bool has_encoder = false;
        range_encoder_desc desc{};
        EncArgs args{};
        size_t lds_bytes = 0;
        size_t lds_base = 0;     // LDS of the encoder without the power table of the faithful SH mode
        DevBuf<int32_t> d_slot_base;
        DevBuf<double> d_coefA, d_coefB, d_seedc;
        DevBuf<double> d_wp[ENC_MAX_LAYERS], d_bias[ENC_MAX_LAYERS];
        DevBuf<SHDesc> d_sh_desc;
        DevBuf<double> d_sh_coef;
        DevBuf<int32_t> d_sh_pow;
        DevBuf<double> ws_h1, ws_h1a, ws_h2, ws_e3;   // the small-batch kernels' activations
        DevBuf<uint32_t> ws_enc_sync;   // encoder_tile_kernel: 4 phase counters, 64 words apart
    } enc;
    struct Bank {
        bool has_bank = false;
        bool has_values = false;         // false: keys-only bank (range_set_keys): top-k side channel only
        int64_t n_rows = 0, n_pad = 0, row_offset = 0;
        DevBuf<float> d_keys, d_values, d_xyz4;
        DevBuf<uint32_t> d_keys_bf16;    // bf16 copy of the keys in MFMA fragment order (8 KB per 16 rows)
        DevBuf<uint32_t> d_keys_f16;     // fp16 copy x tg_key_scale, same order: the batch top-k's (built on its first call)
        float tg_key_scale = 0.f;        // 0: not built for the current keys
        float key_norm_max = 1.f;        // largest |key row| (error bound of the prefilter)
        float xyz_norm_max = 1.f;        // largest |location row| (the geo head's logits must be <= 1 too)
        // opt-in pass 2 on bf16 planes of the values (attend_bf16x3.h): RANGE_PV_EXACT unless asked for
        int pv_mode = RANGE_PV_EXACT;
        DevBuf<uint32_t> d_vplanes;      // (ceil(n_rows/32), 4 pieces, 16 tiles, 3 planes, 64 lanes, 8 bf16)
        int64_t vplanes_groups = 0;
    } bank;
    // range_set_temperatures: the temperatures range_forward / range_forward_host run at (0: the model's default)
    float tau_sem_set = 0.f, tau_geo_set = 0.f;
    // the queries of the last call and the workspace of the two passes / the one-pass route
    struct Passes {
        DevBuf<double> ws_ehat64;
        DevBuf<float> ws_ehat32, ws_xq, ws_stats;
        int64_t ws_queries = 0;          // queries whose e-hat the workspace holds (range_forward* / range_encode_raw): range_topk_last
        DevBuf<float> ws_stats_parts, ws_slabs;
        DevBuf<float> ws_small_o, ws_small_z;    // attend_small_kernel: per-workgroup partial products / weight sums
        int last_qtiles = 0, last_splits = 0;    // range_last_attend_geometry
    } pass;
    // logits kept by the last range_scan_stats(keep_logits = 1): kept_B queries x kept_blocks
    // bank blocks, 1 KB tiles (scan_common.h: logit_tile); kept_B == 0: nothing kept
    struct Kept {
        DevBuf<float> ws_logits, ws_rowmax, ws_theta;
        DevBuf<float> ws_stat_parts;     // range_stats_kept: the per-split parts of one launch's pairs
        int64_t kept_B = 0, kept_total = 0;
        int32_t kept_blocks = 0;
        bool warned_no_keep = false;
    } kept;
    struct Topk {
        DevBuf<float> ws_cand_val;
        DevBuf<int32_t> ws_cand_idx;             // pass 1's candidates (in-scan lists / from the kept logits)
        DevBuf<unsigned long long> ws_cand_keys;
        DevBuf<float> ws_cand_dmax;
        DevBuf<int32_t> ws_exact_count;          // queries range_topk_stream recomputed by brute force
        DevBuf<uint32_t> ws_topk_sync;           // TOPKS_SYNC_WORDS: 8 arrival counters (they only count up), key-norm scratch
        uint32_t topk_sync_base[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // what the counters read when the next fused launch starts
        DevBuf<float> ws_tg_gmax, ws_tg_theta;   // topk_gemm.h: group maxima (n_splits * 2, B, 4), thresholds (B)
        DevBuf<uint32_t> ws_tg_qfrag;            // ... the call's queries as fp16 fragments (512 B per query)
        DevBuf<float> ws_tg_qscale;              // ... and their scales
        DevBuf<uint32_t> ws_tg_cnt, ws_tg_ovf;
        DevBuf<uint2> ws_tg_cand;                // candidate lists: lengths (B, lists), rows (B, lists, TG_CAP_L); overflow flags (B)
        DevBuf<uint32_t> ws_read_sink;           // range_stream_read_timed: one word per workgroup
    } topk;
    // range_posenc_features: the frequency tables seen so far, each in device memory of its own (a table
    // is never overwritten: a launch in flight on another stream may still read it)
    struct Posenc {
        struct Table { std::vector<double> host; DevBuf<double> dev; };
        std::vector<std::unique_ptr<Table>> tables;
    } posenc;
    // range_set_csp: the installed CSP network - its plan (for B = 1), the packed parameters, the frequencies
    struct Csp {
        bool has = false;
        int kind = 0, F = 0, act = 0;
        bool skip = false, layn = false;
        int widths[CSP_MAX_LAYERS] = {};
        CspPlan plan;
        DevBuf<float> d_params;
        DevBuf<double> d_freq;
        DevBuf<CspLayerArgs> d_layers;
        // range_set_csp_head: the packed class_emb (csp_pack_head); range_csp_predict: a chunk's embeddings
        int num_classes = 0;             // 0: no head
        DevBuf<float> d_head;
        DevBuf<float> ws_feats;
        // range_csp_rank: the parts' partial results of a split sweep (csp_rank_kernel.h), in doubles
        DevBuf<double> ws_rank;
    } csp;
    // range_nearest_support: the chunks' partial (a, index) pairs of a split scan (checker_kernel.h)
    struct Checker {
        DevBuf<double> ws_a;
        DevBuf<int64_t> ws_idx;
    } checker;
    // range_set_neighbors: the packed training set of the neighbour / grid geo priors (neighbor_kernel.h), the
    // chunks' partial count rows of a split scan, the selection of a k-nearest-neighbour call.  range_set_kde_points
    // installs a WEIGHTED set in the same slot (kde_kernel.h): the bins, their counts in the points' cell word
    struct Neighbors {
        int64_t N = 0;                   // 0: no set installed
        int C = 0;
        bool hav = false, has_cells = false;
        int kde_bits = 0;                // > 0: a weighted set, the scale bits of its fixed-point sums
        DevBuf<NeighborPoint> d_pts;
        DevBuf<uint64_t> ws_rows;        // a split scan's partial rows of either kind, sized in bytes (plan: ws_bytes)
        DevBuf<double> ws_redk;
        DevBuf<int64_t> ws_jlast;
    } nb;
    // range_headfit_begin: the class head being fitted (headfit_kernels.h) - W and Adam's moments in the packed
    // layout of csp_pack_head, the steps taken, the workspace of a step (host_plan.h: headfit_plan)
    struct Headfit {
        int C = 0, F = 0;                // C == 0: no fit begun
        int64_t steps = 0;
        DevBuf<float> d_w, d_m, d_v;
        DevBuf<float> ws;
    } hf;
    // range_cspfit_begin: the CSP network being trained (cspfit_kernels.h) - every parameter and Adam's two moments at
    // the offsets of host_plan.h: cspfit_plan, the frequencies, the steps taken, the workspace of a step
    struct Cspfit {
        int C = 0;                       // 0: no fit begun
        int kind = 0, F = 0, act = 0, n_layers = 0;
        bool skip = false, layn = false;
        int widths[CSP_MAX_LAYERS] = {};
        int64_t steps = 0;
        size_t store = 0;                // floats of one copy: d_pmv holds the parameters, then m, then v
        DevBuf<float> d_pmv;
        DevBuf<double> d_freq;
        DevBuf<float> ws;
    } cf;
    // words of host memory the kernels can write (hipHostMallocMapped; async_err.h): set by a persistent
    // kernel whose bounded wait for other workgroups gave up; read - without synchronising - by the
    // next call and behind every synchronising exit (check_async_error)
    uint32_t* h_async_err = nullptr;
    uint32_t* d_async_err = nullptr;
    bool debug_giveup_next = false;          // range_debug_raise_async_error: the next persistent launch gives up
    // host contract (range_forward_host): device result, pinned staging, copy stream, copy threads
    struct Host {
        DevBuf<double> ws_out64;
        void* h_stage = nullptr;
        size_t h_stage_bytes = 0;
        hipStream_t copy_stream = nullptr;
        std::unique_ptr<HostCopyPool> pool;
    } host;
    // range_forward in chunks (forward_host.h): the stream of the later chunks' pass 1 and the events between it
    // and the caller's stream - [0] chunk 0 scanned, [i] the statistics of chunk i merged; created on first use
    struct Overlap {
        hipStream_t aux_stream = nullptr;
        std::vector<hipEvent_t> events;
    } ovl;
    // profiling: event pairs per kernel kind
    struct Profiling {
        bool on = false;
        std::vector<std::pair<hipEvent_t, hipEvent_t>> pairs[RANGE_PROF_KINDS];
    } prof;
    std::vector<hipEvent_t> ev_pool;
    hipEvent_t get_event() {
        if (!ev_pool.empty()) { hipEvent_t e = ev_pool.back(); ev_pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
    ~range_ctx() {
        if (host.h_stage) (void)hipHostFree(host.h_stage);
        if (h_async_err) (void)hipHostFree(h_async_err);
        if (host.copy_stream) (void)hipStreamDestroy(host.copy_stream);
        if (ovl.aux_stream) (void)hipStreamDestroy(ovl.aux_stream);
        for (auto e : ovl.events) (void)hipEventDestroy(e);
        for (auto& v : prof.pairs) for (auto& p : v) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
        for (auto e : ev_pool) (void)hipEventDestroy(e);
    }
};

namespace {
// records an event pair around one kernel launch when profiling is on
struct ProfScope {
    range_ctx* c; int which; hipStream_t s; hipEvent_t a = nullptr, b = nullptr;
    ProfScope(range_ctx* c_, int which_, hipStream_t s_) : c(c_), which(which_), s(s_) {
        if (c->prof.on) { a = c->get_event(); b = c->get_event(); if (a) (void)hipEventRecord(a, s); }
    }
    ~ProfScope() {
        if (a && b) { (void)hipEventRecord(b, s); c->prof.pairs[which].emplace_back(a, b); }
    }
};

// the kernel headers' constants that the launch plans take (host_plan.h)
constexpr PlanConsts PLAN_CONSTS{QTILE, BLK, VAL_DIM, MAX_TOPK, P1_WG_PER_CU, ENC_QTILE, TOPKS_WL,
                                 TG_QBLOCK, TG_WG_PER_CU, TG_CAP_L};

// One kernel launch.  A launch with dynamic LDS first raises the kernel's limit to what it asks for
// (on every launch); a launch error comes back as the RANGE_* code.
template <typename... P, typename... A>
int launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, const A&... args) {
    if (lds)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
    HIP_TRY(hipGetLastError());
    return RANGE_OK;
}

// Enqueues `body` once - or, repeats > 1, `repeats` times back to back between ONE pair of events,
// waits for them and writes the time per repetition to *avg_us.
template <typename F>
int timed_repeat(range_ctx* c, hipStream_t s, int repeats, float* avg_us, F&& body) {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (repeats > 1) {
        ev0 = c->get_event();
        ev1 = c->get_event();
        HIP_TRY(hipEventRecord(ev0, s));
    }
    for (int rep = 0; rep < std::max(1, repeats); ++rep)
        if (int rc = body()) return rc;
    if (repeats > 1) {
        HIP_TRY(hipEventRecord(ev1, s));
        HIP_TRY(hipEventSynchronize(ev1));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
        if (avg_us) *avg_us = ms * 1e3f / (float)repeats;
        c->ev_pool.push_back(ev0);
        c->ev_pool.push_back(ev1);
    }
    return RANGE_OK;
}

}  // namespace

// A persistent kernel that gave up waiting for its other workgroups (possible only when something
// else holds the GPU's CUs for seconds) has written NaN rows (encoder) / NaN values and -1 indices
// (top-k) for what it could not finish, and set a word of host memory.  That word is read here - in
// front of the next encoder / top-k call and behind every synchronising exit, without touching the
// stream - and the context takes the separate-launch form of that kernel from then on: co-residency
// of a persistent grid is a precondition the library cannot check, so after one failure it stops
// relying on it (the same branch RANGE_ENC_FUSED=0 / RANGE_TOPKS_FUSED=0 select).
static int check_async_error(range_ctx* c) {
    if (!c->h_async_err) return RANGE_OK;
    volatile uint32_t* w = c->h_async_err;
    const bool enc = w[RANGE_ASYNC_WORD_ENCODER] != 0, topk = w[RANGE_ASYNC_WORD_TOPK] != 0;
    if (!enc && !topk) return RANGE_OK;
    w[RANGE_ASYNC_WORD_ENCODER] = 0;
    w[RANGE_ASYNC_WORD_TOPK] = 0;
    if (enc) c->sw.enc_fused = false;
    if (topk) c->sw.topks_fused = false;
    return fail(RANGE_ERR_HIP, "a persistent %s launch of an earlier call gave up waiting for its workgroups (is another "
                               "process holding the GPU?); the rows it could not finish were written as NaN%s, and this "
                               "context runs that step as separate launches from now on: re-issue the call",
                enc && topk ? "encoder and a top-k" : enc ? "encoder" : "top-k", topk ? " / index -1" : "");
}
