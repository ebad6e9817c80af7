// Host side of the CSP encoder fit (cspfit_kernels.h; include/range_cspfit.h).  Part of range_hip.hip's translation
// unit, behind engine_ctx.h, csp_host.h (the class head's launch) and headfit_host.h (the row checks, the head pass, the
// update launch, Adam's scalars and HEADFIT_STEP / _GRAD / _LOSS, which name what a call does here too).
#pragma once

static void (*cspfit_fwd_row_for(int act))(CspfitRowArgs) {
    static void (*const k[CSP_ACTS])(CspfitRowArgs) = {cspfit_fwd_row_kernel<0>, cspfit_fwd_row_kernel<1>, cspfit_fwd_row_kernel<2>,
                                                      cspfit_fwd_row_kernel<3>, cspfit_fwd_row_kernel<4>};
    return k[act];
}
static void (*cspfit_bwd_row_for(int act))(CspfitRowArgs) {
    static void (*const k[CSP_ACTS])(CspfitRowArgs) = {cspfit_bwd_row_kernel<0>, cspfit_bwd_row_kernel<1>, cspfit_bwd_row_kernel<2>,
                                                      cspfit_bwd_row_kernel<3>, cspfit_bwd_row_kernel<4>};
    return k[act];
}

static CspfitPlan cspfit_plan_of(const range_ctx::Cspfit& f, int64_t R, int64_t max_grid, int32_t panel_cols) {
    return cspfit_plan(f.kind, f.F, f.n_layers, f.widths, f.skip, f.layn, f.C, R, max_grid, panel_cols);
}

// One call on the step's rows: features, the layers forward, the head per class panel (logit gradient, fold, dE, the
// head's update), the loss scalars, then the layers backward (row launch, column sums, dX, dW).
static int cspfit_run(range_ctx* c, int what, const double* lonlat, int64_t N, const int32_t* rows, const int32_t* labels,
                      int32_t B, const double* bg, int32_t Bg, double weight, const HeadfitAdam* adam, double drop_p,
                      uint64_t drop_seed, float* grads, float* loss3, float* emb, int64_t max_grid, int32_t panel_cols,
                      range_stream_t stream) {
    if (!c || !lonlat || !labels) return fail(RANGE_ERR_INVALID, "null argument");
    range_ctx::Cspfit& f = c->cf;
    if (!f.C) return fail(RANGE_ERR_STATE, "no CSP fit begun (range_cspfit_begin)");
    if (what == HEADFIT_GRAD && !grads) return fail(RANGE_ERR_INVALID, "null argument");
    if (what == HEADFIT_LOSS && !loss3 && !emb) return fail(RANGE_ERR_INVALID, "null argument");
    if (int rc = headfit_check_rows(N, rows, B, bg, Bg, weight, true)) return rc;
    if (!(drop_p >= 0.0 && drop_p < 1.0)) return fail(RANGE_ERR_INVALID, "dropout_p must be in [0, 1)");
    if (!aligned(lonlat, 8) || !aligned(bg, 8) || !aligned(rows, 4) || !aligned(labels, 4) || !aligned(grads, 4) || !aligned(loss3, 4) ||
        !aligned(emb, 4))
        return fail(RANGE_ERR_INVALID, "the device pointers must be aligned to their element");
    const int64_t R = (int64_t)B + Bg;
    const CspfitPlan p = cspfit_plan_of(f, R, max_grid, panel_cols);
    if (!p.valid) return fail(RANGE_ERR_INVALID, "B = %d, Bg = %d: %s", B, Bg, p.why);
    HeadfitUpdateArgs u{};
    const bool step = what == HEADFIT_STEP;
    if (step)
        if (int rc = headfit_adam_scalars(*adam, f.steps, u)) return rc;
    ENTER_DEVICE(c);
    if (f.ws.ensure(p.ws_floats) != hipSuccess) return fail(RANGE_ERR_NOMEM, "out of device memory (%zu bytes of workspace)", p.ws_bytes);
    const hipStream_t s = (hipStream_t)stream;
    float* const ws = f.ws.p;
    float* const prm = f.d_pmv.p;
    const int64_t m_delta = (int64_t)f.store, v_delta = 2 * (int64_t)f.store;
    const int L = p.n_layers, nf = p.net.out_width;
    // dropout: the threshold on 24 bits, the scale, the per-layer keys
    const bool drop_on = drop_p > 0.0;
    const uint32_t thresh = (uint32_t)std::floor((1.0 - drop_p) * 16777216.0);
    const float drop_scale = (float)(1.0 / (1.0 - drop_p));
    const uint32_t key0 = cspfit_mix(cspfit_mix(cspfit_mix((uint32_t)drop_seed) ^ (uint32_t)(drop_seed >> 32)) ^ (uint32_t)f.steps);
    auto row_args = [&](int l) {
        const CspLayerPlan& lp = p.net.layer[l];
        CspfitRowArgs r{};
        r.z = ws + p.z_off[l];
        r.xin = lp.skip ? ws + p.x_off[l] : nullptr;
        r.bias = prm + p.b_off[l];
        r.gamma = lp.layn ? prm + p.g_off[l] : nullptr;
        r.beta = lp.layn ? prm + p.be_off[l] : nullptr;
        r.R = (int32_t)R;
        r.n = lp.out;
        r.lpr = p.lpr;
        r.drop_on = drop_on;
        r.drop_key = cspfit_mix(key0 ^ (uint32_t)l);
        r.drop_thresh = thresh;
        r.drop_scale = drop_scale;
        return r;
    };
    // ---- forward
    if (int rc = launch(cspfit_features_kernel, dim3(p.feat_grid), dim3(p.block), 0, s, (const double*)f.d_freq.p, lonlat, N, rows, B, bg,
                        (int32_t)R, (int32_t)f.F, (int32_t)f.kind, (int32_t)p.net.in0, ws + p.x_off[0]))
        return rc;
    for (int l = 0; l < L; ++l) {
        if (int rc = csp_head_launch(p.fwd(l), ws + p.x_off[l], prm + p.w_off[l], nullptr, ws + p.z_off[l], R, s)) return rc;
        CspfitRowArgs r = row_args(l);
        r.y = ws + p.x_off[l + 1];
        if (int rc = launch(cspfit_fwd_row_for(f.act), dim3(p.row_grid), dim3(p.block), 0, s, r)) return rc;
    }
    float* const E = ws + p.x_off[L];
    if (emb) HIP_TRY(hipMemcpyAsync(emb, E, (size_t)R * nf * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (what == HEADFIT_LOSS && !loss3) return RANGE_OK;
    // ---- the head (headfit_host.h), with dE = G W_c behind every panel's gradient, before the panel's update: the
    // product reads the panel's columns of W_c as the step found them
    const HeadfitPlan& hp = p.head;
    float* const wc = prm + p.c_off;
    float* const g = ws + p.g_ws_off;
    float* dy[2] = {ws + p.dy_off[0], ws + p.dy_off[1]};
    auto back_head = [&](int pn, int tile0, int n_tiles) {
        CspfitBackArgs b{};
        b.a = g;
        b.w = wc;
        b.out = dy[0];
        b.n_items = p.back_items(nf);
        b.R = (int32_t)R;
        b.lda = hp.panel_cols;
        b.c0 = tile0 * 32;
        b.kc = std::min(n_tiles * 32, f.C - b.c0);
        b.k_groups = hp.k_groups;
        b.N = nf;
        b.col_groups = p.back_col_groups(nf);
        b.first = pn == 0;
        return launch(cspfit_back_kernel, dim3(p.back_grid(nf)), dim3(p.block), 0, s, b);
    };
    if (int rc = headfit_head_pass(what, hp, E, wc, wc + m_delta, wc + v_delta, g, ws + p.part_off, ws + p.rowsum_off, labels, B, Bg, weight,
                                   u, what == HEADFIT_GRAD ? grads + p.uc_off : nullptr, loss3, nullptr, s, back_head))
        return rc;
    if (what == HEADFIT_LOSS) return RANGE_OK;
    // ---- the layers backward; dy[cur] holds the gradient of layer l's output
    int cur = 0;
    for (int l = L - 1; l >= 0; --l) {
        const CspLayerPlan& lp = p.net.layer[l];
        float* const dz = ws + p.dz_off;
        float* const dyx = ws + p.dyx_off;
        CspfitRowArgs r = row_args(l);
        r.dy = dy[cur];
        r.dz = dz;
        r.ds = lp.skip ? dy[1 - cur] : nullptr;
        r.dyx = lp.layn ? dyx : nullptr;
        if (int rc = launch(cspfit_bwd_row_for(f.act), dim3(p.row_grid), dim3(p.block), 0, s, r)) return rc;
        CspfitColsumArgs cs{};
        cs.src0 = dz; cs.src1 = dyx; cs.src2 = dy[cur];
        cs.p0 = prm + p.b_off[l]; cs.p1 = prm + p.g_off[l]; cs.p2 = prm + p.be_off[l];
        if (what == HEADFIT_GRAD) { cs.out0 = grads + p.ub_off[l]; cs.out1 = grads + p.ug_off[l]; cs.out2 = grads + p.ube_off[l]; }
        cs.m_delta = m_delta; cs.v_delta = v_delta;
        cs.R = (int32_t)R; cs.n = lp.out; cs.kinds = p.colsum_kinds(l);
        cs.adam = u;
        if (int rc = launch(step ? cspfit_colsum_kernel<true> : cspfit_colsum_kernel<false>, dim3(p.colsum_grid(l)),
                            dim3(CSPFIT_COLSUM_BLOCK), 0, s, cs))
            return rc;
        const HeadfitPlan up = p.upd(l);
        if (l > 0) {                     // dX = dZ W (+ dS), from the weights this step started from
            CspfitBackArgs b{};
            b.a = dz;
            b.w = prm + p.w_off[l];
            b.addend = lp.skip ? dy[1 - cur] : nullptr;
            b.out = dy[1 - cur];
            b.n_items = p.back_items(lp.in);
            b.R = (int32_t)R;
            b.lda = lp.out;
            b.c0 = 0;
            b.kc = lp.out;
            b.k_groups = up.k_groups;
            b.N = lp.in;
            b.col_groups = p.back_col_groups(lp.in);
            b.first = 1;
            if (int rc = launch(cspfit_back_kernel, dim3(p.back_grid(lp.in)), dim3(p.block), 0, s, b)) return rc;
        }
        float* const w = prm + p.w_off[l];
        if (int rc = headfit_update_launch(step, u, ws + p.x_off[l], dz, w, w + m_delta, w + v_delta,
                                           what == HEADFIT_GRAD ? grads + p.uw_off[l] : nullptr, up, 0, lp.out, s))   // (dZ's row stride)
            return rc;
        cur = 1 - cur;
    }
    if (step) ++f.steps;
    return RANGE_OK;
}

extern "C" {

int range_cspfit_plan(int32_t kind, int32_t F, int32_t n_layers, const int32_t* widths, int32_t skip, int32_t use_layn, int32_t C,
                      int64_t rows, int64_t max_grid, int32_t panel_cols, int64_t* out16) {
    if (!widths || !out16) return fail(RANGE_ERR_INVALID, "null argument");
    if (n_layers < 1 || n_layers > CSP_MAX_LAYERS)
        return fail(RANGE_ERR_INVALID, "%d linear layers (1 .. %d: at most 8 hidden layers)", n_layers, CSP_MAX_LAYERS);
    int w[CSP_MAX_LAYERS];
    for (int i = 0; i < n_layers; ++i) w[i] = widths[i];
    const CspfitPlan p = cspfit_plan(kind, F, n_layers, w, skip != 0, use_layn != 0, C, rows, max_grid, panel_cols);
    if (!p.valid) return fail(RANGE_ERR_INVALID, "CSP fit outside the supported envelope: %s", p.why);
    const int64_t out[16] = {p.head.panel_cols, p.head.n_panels, p.head.tile_rows, p.lpr, (int64_t)p.feat_grid, (int64_t)p.row_grid,
                             (int64_t)p.back_grid(p.net.out_width), (int64_t)p.head.grad_grid(0), (int64_t)p.head.update_grid(0),
                             (int64_t)p.lds_bytes, (int64_t)p.ws_bytes, (int64_t)p.n_params, (int64_t)p.store_floats, p.widest, 0, 0};
    std::copy(out, out + 16, out16);
    return RANGE_OK;
}

int range_cspfit_begin(range_ctx* c, int32_t kind, const double* freq_host, int32_t F, int32_t n_layers, const int32_t* widths,
                       const float* const* weights, const float* const* biases, const float* const* ln_gamma,
                       const float* const* ln_beta, int32_t act, int32_t skip, int32_t use_layn, const float* class_emb, int32_t C) {
    if (!c || !freq_host || !widths || !weights || !biases) return fail(RANGE_ERR_INVALID, "null argument");
    if (act < 0 || act >= CSP_ACTS) return fail(RANGE_ERR_INVALID, "activation %d", act);
    if (n_layers < 1 || n_layers > CSP_MAX_LAYERS)
        return fail(RANGE_ERR_INVALID, "%d linear layers (1 .. %d: at most 8 hidden layers)", n_layers, CSP_MAX_LAYERS);
    int w[CSP_MAX_LAYERS];
    for (int i = 0; i < n_layers; ++i) w[i] = widths[i];
    const CspfitPlan p = cspfit_plan(kind, F, n_layers, w, skip != 0, use_layn != 0, C, 1);
    if (!p.valid) return fail(RANGE_ERR_INVALID, "CSP fit outside the supported envelope: %s", p.why);
    for (int i = 0; i < n_layers; ++i) {
        if (!weights[i] || !biases[i]) return fail(RANGE_ERR_INVALID, "null parameters of layer %d", i);
        if (p.net.layer[i].layn && (!ln_gamma || !ln_beta || !ln_gamma[i] || !ln_beta[i]))
            return fail(RANGE_ERR_INVALID, "null LayerNorm parameters of layer %d", i);
    }
    std::vector<float> store(3 * p.store_floats, 0.0f);
    for (int i = 0; i < n_layers; ++i) {
        const CspLayerPlan& l = p.net.layer[i];
        csp_pack_head(csp_head_plan(l.in, l.out, l.out, 1, CSP_HEAD_PROBS), weights[i], store.data() + p.w_off[i]);
        std::copy(biases[i], biases[i] + l.out, store.data() + p.b_off[i]);
        if (l.layn) {
            std::copy(ln_gamma[i], ln_gamma[i] + l.out, store.data() + p.g_off[i]);
            std::copy(ln_beta[i], ln_beta[i] + l.out, store.data() + p.be_off[i]);
        }
    }
    if (class_emb) csp_pack_head(csp_head_plan(p.net.out_width, C, C, 1, CSP_HEAD_PROBS), class_emb, store.data() + p.c_off);
    ENTER_DEVICE(c);
    HIP_TRY(hipDeviceSynchronize());         // a launch in flight may still use the fit this call replaces
    range_ctx::Cspfit& f = c->cf;
    f.C = 0;
    HIP_TRY(f.d_pmv.upload(store));
    HIP_TRY(f.d_freq.upload(std::vector<double>(freq_host, freq_host + F)));
    f.kind = kind;
    f.F = F;
    f.act = act;
    f.n_layers = n_layers;
    f.skip = skip != 0;
    f.layn = use_layn != 0;
    std::copy(w, w + n_layers, f.widths);
    f.store = p.store_floats;
    f.steps = 0;
    f.C = C;
    return RANGE_OK;
}

int32_t range_cspfit_classes(const range_ctx* c) { return c ? c->cf.C : 0; }
int32_t range_cspfit_width(const range_ctx* c) { return c && c->cf.C ? c->cf.widths[c->cf.n_layers - 1] : 0; }
int64_t range_cspfit_steps(const range_ctx* c) { return c && c->cf.C ? c->cf.steps : 0; }
int64_t range_cspfit_param_count(const range_ctx* c) { return c && c->cf.C ? (int64_t)cspfit_plan_of(c->cf, 1, 0, 0).n_params : 0; }

int range_cspfit_step_grid(range_ctx* c, const double* lonlat, int64_t N, const int32_t* rows, const int32_t* labels, int32_t B,
                           const double* bg, int32_t Bg, double rand_sample_weight, double lr, double beta1, double beta2, double eps,
                           double weight_decay, double dropout_p, uint64_t dropout_seed, float* loss3, int64_t max_grid,
                           int32_t panel_cols, range_stream_t stream) {
    const HeadfitAdam adam{lr, beta1, beta2, eps, weight_decay};
    return cspfit_run(c, HEADFIT_STEP, lonlat, N, rows, labels, B, bg, Bg, rand_sample_weight, &adam, dropout_p, dropout_seed, nullptr,
                      loss3, nullptr, max_grid, panel_cols, stream);
}

int range_cspfit_step(range_ctx* c, const double* lonlat, int64_t N, const int32_t* rows, const int32_t* labels, int32_t B,
                      const double* bg, int32_t Bg, double rand_sample_weight, double lr, double beta1, double beta2, double eps,
                      double weight_decay, double dropout_p, uint64_t dropout_seed, float* loss3, range_stream_t stream) {
    return range_cspfit_step_grid(c, lonlat, N, rows, labels, B, bg, Bg, rand_sample_weight, lr, beta1, beta2, eps, weight_decay,
                                  dropout_p, dropout_seed, loss3, 0, 0, stream);
}

int range_cspfit_grad_grid(range_ctx* c, const double* lonlat, int64_t N, const int32_t* rows, const int32_t* labels, int32_t B,
                           const double* bg, int32_t Bg, double rand_sample_weight, double dropout_p, uint64_t dropout_seed,
                           float* grads, float* loss3, int64_t max_grid, int32_t panel_cols, range_stream_t stream) {
    return cspfit_run(c, HEADFIT_GRAD, lonlat, N, rows, labels, B, bg, Bg, rand_sample_weight, nullptr, dropout_p, dropout_seed, grads,
                      loss3, nullptr, max_grid, panel_cols, stream);
}

int range_cspfit_grad(range_ctx* c, const double* lonlat, int64_t N, const int32_t* rows, const int32_t* labels, int32_t B,
                      const double* bg, int32_t Bg, double rand_sample_weight, double dropout_p, uint64_t dropout_seed, float* grads,
                      float* loss3, range_stream_t stream) {
    return range_cspfit_grad_grid(c, lonlat, N, rows, labels, B, bg, Bg, rand_sample_weight, dropout_p, dropout_seed, grads, loss3, 0,
                                  0, stream);
}

int range_cspfit_loss(range_ctx* c, const double* lonlat, int64_t N, const int32_t* rows, const int32_t* labels, int32_t B,
                      const double* bg, int32_t Bg, double rand_sample_weight, double dropout_p, uint64_t dropout_seed, float* loss3,
                      float* emb, range_stream_t stream) {
    return cspfit_run(c, HEADFIT_LOSS, lonlat, N, rows, labels, B, bg, Bg, rand_sample_weight, nullptr, dropout_p, dropout_seed, nullptr,
                      loss3, emb, 0, 0, stream);
}

int range_cspfit_params(range_ctx* c, float* params, range_stream_t stream) {
    if (!c || !params) return fail(RANGE_ERR_INVALID, "null argument");
    const range_ctx::Cspfit& f = c->cf;
    if (!f.C) return fail(RANGE_ERR_STATE, "no CSP fit begun (range_cspfit_begin)");
    if (!aligned(params, 4)) return fail(RANGE_ERR_INVALID, "the device pointer must be 4-byte aligned");
    const CspfitPlan p = cspfit_plan_of(f, 1, 0, 0);
    ENTER_DEVICE(c);
    const hipStream_t s = (hipStream_t)stream;
    const float* const prm = f.d_pmv.p;
    for (int l = 0; l <= p.n_layers; ++l) {
        const bool head = l == p.n_layers;
        const int out = head ? f.C : p.out(l), in = head ? p.net.out_width : p.in(l);
        const HeadfitPlan hp = headfit_plan(out, in, 1);
        if (int rc = launch(headfit_unpack_kernel, dim3(hp.unpack_grid), dim3(hp.block), 0, s, prm + (head ? p.c_off : p.w_off[l]),
                            (int32_t)out, (int32_t)in, (int32_t)hp.k_groups, params + (head ? p.uc_off : p.uw_off[l])))
            return rc;
        if (head) break;
        HIP_TRY(hipMemcpyAsync(params + p.ub_off[l], prm + p.b_off[l], out * sizeof(float), hipMemcpyDeviceToDevice, s));
        if (p.net.layer[l].layn) {
            HIP_TRY(hipMemcpyAsync(params + p.ug_off[l], prm + p.g_off[l], out * sizeof(float), hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(params + p.ube_off[l], prm + p.be_off[l], out * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
    }
    return RANGE_OK;
}

}  // extern "C"
