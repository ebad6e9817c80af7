// Host side of the CSP encoders, their class head and its evaluation (csp_kernel.h, csp_head_kernel.h, csp_rank_kernel.h).
// Part of range_hip.hip's translation unit, behind engine_ctx.h.
#pragma once

// ---- the CSP location encoders (csp_kernel.h), by tile height (32 m_tiles rows) and activation
static void (*csp_kernel_for(int m_tiles, int act))(CspArgs) {
    static void (*const csp_kernels[2][CSP_ACTS])(CspArgs) = {
        {csp_encode_kernel<1, 0>, csp_encode_kernel<1, 1>, csp_encode_kernel<1, 2>, csp_encode_kernel<1, 3>, csp_encode_kernel<1, 4>},
        {csp_encode_kernel<2, 0>, csp_encode_kernel<2, 1>, csp_encode_kernel<2, 2>, csp_encode_kernel<2, 3>, csp_encode_kernel<2, 4>}};
    return csp_kernels[m_tiles - 1][act];
}

// ---- the CSP class head (csp_head_kernel.h), by tile height and output
static void (*csp_head_kernel_for(int m_tiles, int mode))(CspHeadArgs) {
    static void (*const csp_head_kernels[2][CSP_HEAD_MODES])(CspHeadArgs) = {
        {csp_head_kernel<1, 0>, csp_head_kernel<1, 1>, csp_head_kernel<1, 2>},
        {csp_head_kernel<2, 0>, csp_head_kernel<2, 1>, csp_head_kernel<2, 2>}};
    return csp_head_kernels[m_tiles - 1][mode];
}

// One launch of it by plan `p`, in the plan's mode: the B rows of x against the packed w, columns `ids` or all, into
// out.  Shared with the layers' forward products of the CSP encoder fit (cspfit_host.h).
static int csp_head_launch(const CspHeadPlan& p, const float* x, const float* w, const int32_t* ids, float* out, int64_t B,
                           hipStream_t s) {
    CspHeadArgs a{};
    a.x = x;
    a.w4 = reinterpret_cast<const float4*>(w);
    a.ids = ids;
    a.out = out;
    a.B = B;
    a.n_items = p.n_items;
    a.K = p.num_filts;
    a.k_groups = p.k_groups;
    a.ld = p.ld;
    a.M = p.M;
    a.col_tiles = p.col_tiles;
    a.n_chunks = p.n_chunks;
    a.num_classes = p.num_classes;
    a.chunks_per_item = p.chunks_per_item;
    a.groups = p.groups;
    return launch(csp_head_kernel_for(p.m_tiles, p.mode), dim3(p.grid), dim3(p.block), p.lds_bytes, s, a);
}

// ---- the evaluation behind the head (csp_rank_kernel.h), by tile height, image predictions and embeddings
static void (*csp_rank_kernel_for(int m_tiles, int img_kind, bool has_head))(CspRankArgs) {
    static void (*const with_head[2][CSP_IMG_KINDS])(CspRankArgs) = {
        {csp_rank_kernel<1, 0, true>, csp_rank_kernel<1, 1, true>, csp_rank_kernel<1, 2, true>},
        {csp_rank_kernel<2, 0, true>, csp_rank_kernel<2, 1, true>, csp_rank_kernel<2, 2, true>}};
    static void (*const without[CSP_IMG_KINDS])(CspRankArgs) = {nullptr, csp_rank_kernel<2, 1, false>,
                                                                csp_rank_kernel<2, 2, false>};
    return has_head ? with_head[m_tiles - 1][img_kind] : without[img_kind];
}

// the refusals of a call without the network / without the head behind it
static int need_csp(const range_ctx* c) {
    return c->csp.has ? RANGE_OK : fail(RANGE_ERR_INVALID, "no CSP network set (range_set_csp)");
}
static int need_csp_head(const range_ctx* c) {
    return c->csp.has && c->csp.num_classes ? RANGE_OK : fail(RANGE_ERR_INVALID, "no CSP class head set (range_set_csp_head)");
}

// image predictions and their kind agree: a pointer with CSP_IMG_F32 / CSP_IMG_F64, none with CSP_IMG_NONE
static int check_img_kind(const void* img, int32_t img_kind) {
    if (img_kind < 0 || img_kind >= CSP_IMG_KINDS) return fail(RANGE_ERR_INVALID, "img_kind %d", img_kind);
    if ((img != nullptr) != (img_kind != CSP_IMG_NONE))
        return fail(RANGE_ERR_INVALID, "img_kind %d %s image predictions", img_kind, img ? "with" : "without");
    return RANGE_OK;
}

// The composed calls, in chunks of csp_predict_chunk rows (host_plan.h): a chunk is encoded into ws_feats, then
// `body(first_row, n_rows)` enqueues what reads it on the same stream.  The first non-zero code ends the walk.
template <typename Body>
static int csp_for_each_chunk(range_ctx* c, const double* lonlat, int64_t B, range_stream_t stream, Body&& body) {
    const int64_t width = c->csp.plan.out_width, chunk = csp_predict_chunk((int)width);
    ENTER_DEVICE(c);
    if (c->csp.ws_feats.ensure((size_t)(std::min(B, chunk) * width)) != hipSuccess)
        return fail(RANGE_ERR_NOMEM, "out of device memory (%lld bytes of embeddings)", (long long)(std::min(B, chunk) * width * 4));
    for (int64_t i = 0; i < B; i += chunk) {
        const int64_t n = std::min(chunk, B - i);
        if (int rc = range_csp_encode_grid(c, lonlat + 2 * i, n, c->csp.ws_feats.p, 0, stream)) return rc;
        if (int rc = body(i, n)) return rc;
    }
    return RANGE_OK;
}

extern "C" {

int range_set_csp(range_ctx* c, int32_t kind, const double* freq_host, int32_t F, int32_t n_layers, const int32_t* widths,
                  const float* const* weights, const float* const* biases, const float* const* ln_gamma,
                  const float* const* ln_beta, int32_t act, int32_t skip, int32_t use_layn) {
    if (!c || !freq_host || !widths || !weights || !biases) return fail(RANGE_ERR_INVALID, "null argument");
    if (act < 0 || act >= CSP_ACTS) return fail(RANGE_ERR_INVALID, "activation %d", act);
    if (n_layers < 1 || n_layers > CSP_MAX_LAYERS)
        return fail(RANGE_ERR_INVALID, "%d linear layers (1 .. %d: at most 8 hidden layers)", n_layers, CSP_MAX_LAYERS);
    int w[CSP_MAX_LAYERS];
    for (int i = 0; i < n_layers; ++i) w[i] = widths[i];
    const CspPlan p = csp_plan(kind, F, n_layers, w, skip != 0, use_layn != 0, 1);
    if (!p.valid) return fail(RANGE_ERR_INVALID, "CSP network outside the supported envelope: %s", p.why);
    for (int i = 0; i < n_layers; ++i) {
        if (!weights[i] || !biases[i]) return fail(RANGE_ERR_INVALID, "null parameters of layer %d", i);
        if (p.layer[i].layn && (!ln_gamma || !ln_beta || !ln_gamma[i] || !ln_beta[i]))
            return fail(RANGE_ERR_INVALID, "null LayerNorm parameters of layer %d", i);
    }
    std::vector<float> packed(p.packed_floats, 0.0f);
    for (int i = 0; i < n_layers; ++i)
        csp_pack_layer(p, i, weights[i], biases[i], p.layer[i].layn ? ln_gamma[i] : nullptr,
                       p.layer[i].layn ? ln_beta[i] : nullptr, packed.data());
    ENTER_DEVICE(c);
    // a launch in flight on any stream may still read the parameters this call replaces
    HIP_TRY(hipDeviceSynchronize());
    c->csp.has = false;
    c->csp.num_classes = 0;          // a head belongs to the network it was installed behind
    HIP_TRY(c->csp.d_params.upload(packed));
    HIP_TRY(c->csp.d_freq.upload(std::vector<double>(freq_host, freq_host + F)));
    std::vector<CspLayerArgs> layers;
    for (int i = 0; i < n_layers; ++i) {
        const CspLayerPlan& l = p.layer[i];
        layers.push_back(CspLayerArgs{l.out, l.n_tiles, l.k_groups, l.skip, l.layn, (uint32_t)l.w_off, (uint32_t)l.b_off,
                                      (uint32_t)l.g_off, (uint32_t)l.be_off});
    }
    HIP_TRY(c->csp.d_layers.upload(layers));
    c->csp.kind = kind;
    c->csp.F = F;
    c->csp.act = act;
    c->csp.skip = skip != 0;
    c->csp.layn = use_layn != 0;
    std::copy(w, w + n_layers, c->csp.widths);
    c->csp.plan = p;
    c->csp.has = true;
    return RANGE_OK;
}

int32_t range_csp_width(const range_ctx* c) { return c && c->csp.has ? c->csp.plan.out_width : 0; }

int32_t range_csp_tile_rows(const range_ctx* c) { return c && c->csp.has ? c->csp.plan.tile_rows : 0; }

int range_csp_encode_grid(range_ctx* c, const double* lonlat, int64_t B, float* out, int64_t max_grid,
                          range_stream_t stream) {
    if (!c || !lonlat || !out) return fail(RANGE_ERR_INVALID, "null argument");
    if (int rc = need_csp(c)) return rc;
    if (B <= 0) return fail(RANGE_ERR_INVALID, "B must be > 0");
    if (max_grid < 0) return fail(RANGE_ERR_INVALID, "max_grid must be >= 0");
    if (!aligned(lonlat, 8) || !aligned(out, 4))
        return fail(RANGE_ERR_INVALID, "lonlat_dev must be 8-byte aligned, out_dev 4-byte aligned");
    const range_ctx::Csp& m = c->csp;
    const CspPlan p = csp_plan(m.kind, m.F, m.plan.n_layers, m.widths, m.skip, m.layn, B, max_grid);
    if (!p.valid) return fail(RANGE_ERR_INVALID, "B = %lld locations: %s", (long long)B, p.why);
    ENTER_DEVICE(c);
    CspArgs a{};
    a.freq = m.d_freq.p;
    a.lonlat = lonlat;
    a.params = m.d_params.p;
    a.out = out;
    a.B = B;
    a.n_tiles = p.n_tiles;
    a.F = m.F;
    a.kind = m.kind;
    a.layer = m.d_layers.p;
    a.n_layers = p.n_layers;
    a.ld = p.ld;
    a.in0 = p.in0;
    a.in0_pad = p.layer[0].k_pad();
    return launch(csp_kernel_for(p.m_tiles, m.act), dim3(p.grid), dim3(p.block), p.lds_bytes, (hipStream_t)stream, a);
}

int range_set_csp_head(range_ctx* c, const float* class_emb, int32_t C) {
    if (!c || !class_emb) return fail(RANGE_ERR_INVALID, "null argument");
    if (!c->csp.has) return fail(RANGE_ERR_INVALID, "no CSP network set (range_set_csp): the head needs its num_filts");
    const CspHeadPlan p = csp_head_plan(c->csp.plan.out_width, C, C, 1, CSP_HEAD_PROBS);
    if (!p.valid) return fail(RANGE_ERR_INVALID, "CSP class head outside the supported envelope: %s", p.why);
    std::vector<float> packed(p.packed_floats, 0.0f);
    csp_pack_head(p, class_emb, packed.data());
    ENTER_DEVICE(c);
    HIP_TRY(hipDeviceSynchronize());         // a launch in flight may still read the head this call replaces
    c->csp.num_classes = 0;
    HIP_TRY(c->csp.d_head.upload(packed));
    c->csp.num_classes = C;
    return RANGE_OK;
}

int32_t range_csp_classes(const range_ctx* c) { return c && c->csp.has ? c->csp.num_classes : 0; }

int32_t range_csp_head_cols_per_pass(const range_ctx* c) {
    if (!c || !c->csp.has || !c->csp.num_classes) return 0;
    return csp_head_plan(c->csp.plan.out_width, c->csp.num_classes, c->csp.num_classes, 1, CSP_HEAD_PROBS).cols_per_pass;
}

int range_csp_check_ids(range_ctx* c, const int32_t* ids_host, int32_t M) {
    if (!c || !ids_host) return fail(RANGE_ERR_INVALID, "null argument");
    if (int rc = need_csp_head(c)) return rc;
    if (M < 1) return fail(RANGE_ERR_INVALID, "M must be > 0");
    for (int32_t i = 0; i < M; ++i)
        if (ids_host[i] < 0 || ids_host[i] >= c->csp.num_classes)
            return fail(RANGE_ERR_INVALID, "class id %d (entry %d) outside 0 .. %d", ids_host[i], i, c->csp.num_classes - 1);
    return RANGE_OK;
}

int range_csp_head_grid(range_ctx* c, const float* feats, int64_t B, const int32_t* ids, int32_t M, int32_t mode,
                        float* out, int64_t max_grid, range_stream_t stream) {
    if (!c || !feats || !out) return fail(RANGE_ERR_INVALID, "null argument");
    if (int rc = need_csp_head(c)) return rc;
    if (B <= 0) return fail(RANGE_ERR_INVALID, "B must be > 0");
    if (M < 1) return fail(RANGE_ERR_INVALID, "M must be > 0");
    if (max_grid < 0) return fail(RANGE_ERR_INVALID, "max_grid must be >= 0");
    if (mode < 0 || mode >= CSP_HEAD_MODES) return fail(RANGE_ERR_INVALID, "mode %d", mode);
    if (mode == CSP_HEAD_SUM && ids) return fail(RANGE_ERR_INVALID, "SUM runs over all classes: no class ids");
    if (!ids && M != c->csp.num_classes)
        return fail(RANGE_ERR_INVALID, "M = %d without class ids: the head has %d classes", M, c->csp.num_classes);
    if (!aligned(feats, 4) || !aligned(out, 4) || !aligned(ids, 4))
        return fail(RANGE_ERR_INVALID, "the device pointers must be 4-byte aligned");
    const range_ctx::Csp& m = c->csp;
    const CspHeadPlan p = csp_head_plan(m.plan.out_width, m.num_classes, M, B, mode, max_grid);
    if (!p.valid) return fail(RANGE_ERR_INVALID, "B = %lld, M = %d: %s", (long long)B, M, p.why);
    ENTER_DEVICE(c);
    return csp_head_launch(p, feats, m.d_head.p, ids, out, B, (hipStream_t)stream);
}

int range_csp_head(range_ctx* c, const float* feats, int64_t B, const int32_t* ids, int32_t M, int32_t mode, float* out,
                   range_stream_t stream) {
    return range_csp_head_grid(c, feats, B, ids, M, mode, out, 0, stream);
}

int range_csp_predict(range_ctx* c, const double* lonlat, int64_t B, const int32_t* ids, int32_t M, int32_t mode,
                      float* out, range_stream_t stream) {
    if (!c || !lonlat || !out) return fail(RANGE_ERR_INVALID, "null argument");
    if (int rc = need_csp_head(c)) return rc;
    if (B <= 0) return fail(RANGE_ERR_INVALID, "B must be > 0");
    if (M < 1) return fail(RANGE_ERR_INVALID, "M must be > 0");
    if (mode < 0 || mode >= CSP_HEAD_MODES) return fail(RANGE_ERR_INVALID, "mode %d", mode);
    return csp_for_each_chunk(c, lonlat, B, stream, [&](int64_t i, int64_t n) {
        return range_csp_head_grid(c, c->csp.ws_feats.p, n, ids, M, mode, out + i * (mode == CSP_HEAD_SUM ? 1 : M), 0, stream);
    });
}

int range_csp_rank_grid(range_ctx* c, const float* feats, int64_t B, const void* img, int32_t img_kind, const int32_t* labels,
                        int32_t* greater, int32_t* tied_after, int32_t* argmax, int64_t max_grid, int32_t col_parts,
                        range_stream_t stream) {
    if (!c || !labels || !greater || !tied_after || !argmax) return fail(RANGE_ERR_INVALID, "null argument");
    if (int rc = need_csp_head(c)) return rc;
    if (!feats && !img) return fail(RANGE_ERR_INVALID, "neither embeddings nor image predictions");
    if (int rc = check_img_kind(img, img_kind)) return rc;
    if (B <= 0) return fail(RANGE_ERR_INVALID, "B must be > 0");
    if (max_grid < 0 || col_parts < 0) return fail(RANGE_ERR_INVALID, "max_grid and col_parts must be >= 0");
    if (!aligned(feats, 4) || !aligned(labels, 4) || !aligned(greater, 4) || !aligned(tied_after, 4) || !aligned(argmax, 4) ||
        !aligned(img, img_kind == CSP_IMG_F64 ? 8 : 4))
        return fail(RANGE_ERR_INVALID, "the device pointers must be aligned to their element");
    range_ctx::Csp& m = c->csp;
    const CspRankPlan p = csp_rank_plan(m.plan.out_width, m.num_classes, B, img_kind, feats != nullptr, max_grid, col_parts);
    if (!p.valid) return fail(RANGE_ERR_INVALID, "B = %lld, col_parts = %d: %s", (long long)B, col_parts, p.why);
    ENTER_DEVICE(c);
    CspRankArgs a{};
    a.x = feats;
    a.w4 = reinterpret_cast<const float4*>(m.d_head.p);
    a.img = img;
    a.labels = labels;
    a.greater = greater;
    a.tied = tied_after;
    a.argmax = argmax;
    a.B = B;
    a.n_items = p.n_items;
    a.K = p.num_filts;
    a.k_groups = p.k_groups;
    a.ld = p.ld;
    a.C = p.num_classes;
    a.col_tiles = p.col_tiles;
    a.n_chunks = p.n_chunks;
    a.col_parts = p.col_parts;
    if (p.col_parts > 1) {
        if (m.ws_rank.ensure((p.ws_bytes + 7) / 8) != hipSuccess)
            return fail(RANGE_ERR_NOMEM, "out of device memory (%zu bytes of partial results)", p.ws_bytes);
        const size_t n = (size_t)p.col_parts * (size_t)B;
        a.ws_best = m.ws_rank.p;
        a.ws_greater = reinterpret_cast<int32_t*>(m.ws_rank.p + n);
        a.ws_tied = a.ws_greater + n;
        a.ws_index = a.ws_tied + n;
    }
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = launch(csp_rank_kernel_for(p.m_tiles, img_kind, p.has_head), dim3(p.grid), dim3(p.block), p.lds_bytes, s, a))
        return rc;
    if (p.col_parts == 1) return RANGE_OK;
    return launch(csp_rank_merge_kernel, dim3(p.merge_grid), dim3(p.block), 0, s, a);
}

int range_csp_rank(range_ctx* c, const float* feats, int64_t B, const void* img, int32_t img_kind, const int32_t* labels,
                   int32_t* greater, int32_t* tied_after, int32_t* argmax, range_stream_t stream) {
    return range_csp_rank_grid(c, feats, B, img, img_kind, labels, greater, tied_after, argmax, 0, 0, stream);
}

int range_csp_predict_rank(range_ctx* c, const double* lonlat, int64_t B, const void* img, int32_t img_kind,
                           const int32_t* labels, int32_t* greater, int32_t* tied_after, int32_t* argmax,
                           range_stream_t stream) {
    if (!c || !lonlat || !labels || !greater || !tied_after || !argmax) return fail(RANGE_ERR_INVALID, "null argument");
    if (int rc = need_csp_head(c)) return rc;
    if (B <= 0) return fail(RANGE_ERR_INVALID, "B must be > 0");
    if (int rc = check_img_kind(img, img_kind)) return rc;
    const int64_t row_bytes = c->csp.num_classes * (img_kind == CSP_IMG_F64 ? 8 : 4);     // of the image predictions
    return csp_for_each_chunk(c, lonlat, B, stream, [&](int64_t i, int64_t n) {
        return range_csp_rank_grid(c, c->csp.ws_feats.p, n, img ? static_cast<const char*>(img) + i * row_bytes : nullptr, img_kind,
                                   labels + i, greater + i, tied_after + i, argmax + i, 0, 0, stream);
    });
}

int range_csp_encode(range_ctx* c, const double* lonlat, int64_t B, float* out, range_stream_t stream) {
    return range_csp_encode_grid(c, lonlat, B, out, 0, stream);
}

}  // extern "C"
