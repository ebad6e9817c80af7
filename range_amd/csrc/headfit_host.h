// Host side of the class-head fit (headfit_kernels.h; include/range_headfit.h).  Part of range_hip.hip's translation
// unit, behind engine_ctx.h.  The CSP encoder fit (cspfit_host.h) runs the same row checks, head pass and update launch.
#pragma once

enum { HEADFIT_STEP = 0, HEADFIT_GRAD = 1, HEADFIT_LOSS = 2 };   // what a call of either fit does

struct HeadfitAdam { double lr, beta1, beta2, eps, weight_decay; };

// torch.optim.Adam's scalars of the step behind `steps` taken ones, in double as Python computes them, into `u` - or
// why the hyper-parameters are refused.  Shared with the CSP encoder fit (cspfit_host.h).
static int headfit_adam_scalars(const HeadfitAdam& o, int64_t steps, HeadfitUpdateArgs& u) {
    if (!(o.lr >= 0.0) || !(o.beta1 >= 0.0 && o.beta1 < 1.0) || !(o.beta2 >= 0.0 && o.beta2 < 1.0) || !(o.eps >= 0.0) ||
        !(o.weight_decay >= 0.0) || !std::isfinite(o.lr) || !std::isfinite(o.eps) || !std::isfinite(o.weight_decay))
        return fail(RANGE_ERR_INVALID, "Adam: lr, eps, weight_decay must be finite and >= 0, the betas in [0, 1)");
    const double t = (double)(steps + 1);
    const double bc1 = 1.0 - std::pow(o.beta1, t), bc2 = 1.0 - std::pow(o.beta2, t);
    u.wd = (float)o.weight_decay;
    u.omb1 = (float)(1.0 - o.beta1);
    u.b2 = (float)o.beta2;
    u.omb2 = (float)(1.0 - o.beta2);
    u.eps = (float)o.eps;
    u.step_size = (float)(o.lr / bc1);
    u.bc2_sqrt = (float)std::sqrt(bc2);
    return RANGE_OK;
}

static void (*headfit_grad_kernel_for(int m_tiles, bool write_g))(HeadfitGradArgs) {
    static void (*const kernels[2][2])(HeadfitGradArgs) = {{headfit_grad_kernel<1, false>, headfit_grad_kernel<1, true>},
                                                          {headfit_grad_kernel<2, false>, headfit_grad_kernel<2, true>}};
    return kernels[m_tiles - 1][write_g];
}

// The checks of a step's rows that both fits make; `locations`: the rows are the CSP fit's locations, not features.
static int headfit_check_rows(int64_t N, const int32_t* rows, int32_t B, const void* bg, int32_t Bg, double weight, bool locations) {
    if (N < 1 || B < 1 || Bg < 0) return fail(RANGE_ERR_INVALID, "N and B must be > 0, Bg >= 0");
    if ((bg != nullptr) != (Bg > 0))
        return fail(RANGE_ERR_INVALID, "Bg = %d %s background %s", Bg, bg ? "with" : "without", locations ? "locations" : "rows");
    if (!rows && N < B)
        return fail(RANGE_ERR_INVALID, locations ? "B = %d rows without row ids: there are %lld locations"
                                                 : "B = %d rows without row ids: the feature matrix has %lld", B, (long long)N);
    if (N > (INT64_C(1) << 40)) return fail(RANGE_ERR_INVALID, "N beyond 2^40");
    if (!std::isfinite(weight)) return fail(RANGE_ERR_INVALID, "rand_sample_weight must be finite");
    return RANGE_OK;
}

// One launch of headfit_update_kernel for panel `pn` of plan `p` (its rows, K = p.F, C = p.C): dW = G^T X of the
// panel's classes from x and g (row stride `ldg`), into Adam on (w, m, v) with `u`'s scalars or (`adam` false) into
// dw.  Shared with the layers' dW of the CSP encoder fit.
static int headfit_update_launch(bool adam, HeadfitUpdateArgs u, const float* x, const float* g, float* w, float* m, float* v,
                                 float* dw, const HeadfitPlan& p, int pn, int ldg, hipStream_t s) {
    u.x = x;
    u.g = g;
    u.w = w;
    u.m = m;
    u.v = v;
    u.dw = dw;
    u.n_items = p.update_items(pn);
    u.R = (int32_t)p.rows;
    u.K = p.F;
    u.k_groups = p.k_groups;
    u.C = p.C;
    u.tile0 = p.panel_first_tile(pn);
    u.panel_cols = ldg;
    u.f_groups = p.f_groups;
    return launch(adam ? headfit_update_kernel<true> : headfit_update_kernel<false>, dim3(p.update_grid(pn)), dim3(p.block), 0, s, u);
}

// The head of a step, for both fits, on the p.rows = B + Bg rows of x (p.F wide) and the packed w with its moments:
// per class panel the logit gradient into g, the fold of its row sums (with loss3), `between(pn, tile0, n_tiles)` -
// what the caller enqueues on a panel's G before w changes - and (HEADFIT_STEP: Adam with `u`'s scalars; HEADFIT_GRAD:
// dW stored) the update; then the loss scalars.  `steps`: counted once the panels are enqueued, or null.
template <typename Between>
static int headfit_head_pass(int what, const HeadfitPlan& p, const float* x, float* w, float* m, float* v, float* g, float* parts,
                             float* rowsum, const int32_t* labels, int32_t B, int32_t Bg, double weight, const HeadfitUpdateArgs& u,
                             float* dW, float* loss3, int64_t* steps, hipStream_t s, Between&& between) {
    const int32_t R = (int32_t)p.rows;
    const double bc = (double)B * p.C;
    for (int pn = 0; pn < p.n_panels; ++pn) {
        HeadfitGradArgs a{};
        a.x = x;
        a.w4 = reinterpret_cast<const float4*>(w);
        a.labels = labels;
        a.g = g;
        a.parts = parts;
        a.n_items = p.grad_items(pn);
        a.R = R;
        a.B = B;
        a.K = p.F;
        a.k_groups = p.k_groups;
        a.ld = p.ld;
        a.C = p.C;
        a.tile0 = p.panel_first_tile(pn);
        a.n_tiles = p.panel_n_tiles(pn);
        a.n_chunks = p.grad_chunks(pn);
        a.panel_tiles = p.panel_tiles;
        a.panel_cols = p.panel_cols;
        a.s_neg = (float)(1.0 / bc);
        a.s_lab = (float)(-(double)p.C / bc);
        a.s_bg = Bg ? (float)(weight / ((double)Bg * p.C)) : 0.0f;
        if (int rc = launch(headfit_grad_kernel_for(p.m_tiles, what != HEADFIT_LOSS), dim3(p.grad_grid(pn)), dim3(p.block), p.lds_bytes, s, a))
            return rc;
        if (loss3)
            if (int rc = launch(headfit_fold_kernel, dim3(p.row_grid), dim3(p.block), 0, s, (const float*)parts, rowsum, R, a.n_tiles,
                                a.panel_tiles, (int32_t)(pn == 0)))
                return rc;
        if (what == HEADFIT_LOSS) continue;
        if (int rc = between(pn, a.tile0, a.n_tiles)) return rc;
        if (int rc = headfit_update_launch(what == HEADFIT_STEP, u, x, g, w, m, v, dW, p, pn, p.panel_cols, s)) return rc;
    }
    if (steps) ++*steps;
    if (!loss3) return RANGE_OK;
    return launch(headfit_loss_kernel, dim3(1), dim3(p.block), 0, s, (const float*)rowsum, R, B, (int32_t)p.C, (float)weight, loss3);
}

// One call on the step's rows: the gather, then the head pass.
static int headfit_run(range_ctx* c, int what, const float* feats, int64_t N, const int32_t* rows, const int32_t* labels,
                       int32_t B, const float* bg, int32_t Bg, double weight, const HeadfitAdam* adam, float* dW, float* loss3,
                       int64_t max_grid, int32_t panel_cols, range_stream_t stream) {
    if (!c || !feats || !labels) return fail(RANGE_ERR_INVALID, "null argument");
    range_ctx::Headfit& h = c->hf;
    if (!h.C) return fail(RANGE_ERR_STATE, "no class-head fit begun (range_headfit_begin)");
    if (what == HEADFIT_GRAD && !dW) return fail(RANGE_ERR_INVALID, "null argument");
    if (what == HEADFIT_LOSS && !loss3) return fail(RANGE_ERR_INVALID, "null argument");
    if (int rc = headfit_check_rows(N, rows, B, bg, Bg, weight, false)) return rc;
    if (!aligned(feats, 4) || !aligned(rows, 4) || !aligned(labels, 4) || !aligned(bg, 4) || !aligned(dW, 4) || !aligned(loss3, 4))
        return fail(RANGE_ERR_INVALID, "the device pointers must be 4-byte aligned");
    const int64_t R = (int64_t)B + Bg;
    const HeadfitPlan p = headfit_plan(h.C, h.F, R, max_grid, panel_cols);
    if (!p.valid) return fail(RANGE_ERR_INVALID, "B = %d, Bg = %d: %s", B, Bg, p.why);
    HeadfitUpdateArgs u{};
    if (what == HEADFIT_STEP)
        if (int rc = headfit_adam_scalars(*adam, h.steps, u)) return rc;
    ENTER_DEVICE(c);
    if (h.ws.ensure(p.ws_bytes / sizeof(float)) != hipSuccess)
        return fail(RANGE_ERR_NOMEM, "out of device memory (%zu bytes of workspace)", p.ws_bytes);
    float* const x = h.ws.p;
    float* const g = x + p.x_floats;
    float* const parts = g + p.g_floats;
    float* const rowsum = parts + p.part_floats;
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = launch(headfit_gather_kernel, dim3(p.gather_grid), dim3(p.block), 0, s, feats, N, rows, B, bg, (int32_t)R, (int32_t)h.F, x))
        return rc;
    return headfit_head_pass(what, p, x, h.d_w.p, h.d_m.p, h.d_v.p, g, parts, rowsum, labels, B, Bg, weight, u, dW, loss3,
                             what == HEADFIT_STEP ? &h.steps : nullptr, s, [](int, int, int) { return RANGE_OK; });
}

extern "C" {

int range_headfit_plan(int32_t C, int32_t F, int64_t rows, int64_t max_grid, int32_t panel_cols, int64_t* out8) {
    if (!out8) return fail(RANGE_ERR_INVALID, "null argument");
    const HeadfitPlan p = headfit_plan(C, F, rows, max_grid, panel_cols);
    if (!p.valid) return fail(RANGE_ERR_INVALID, "class-head fit outside the supported envelope: %s", p.why);
    const int64_t out[8] = {p.panel_cols, p.n_panels, p.tile_rows, p.cols_per_pass, (int64_t)p.grad_grid(0), (int64_t)p.update_grid(0),
                            (int64_t)p.lds_bytes, (int64_t)p.ws_bytes};
    std::copy(out, out + 8, out8);
    return RANGE_OK;
}

int range_headfit_begin(range_ctx* c, int32_t C, int32_t F, const float* w0_host) {
    if (!c) return fail(RANGE_ERR_INVALID, "null argument");
    const HeadfitPlan p = headfit_plan(C, F, 1);
    if (!p.valid) return fail(RANGE_ERR_INVALID, "class-head fit outside the supported envelope: %s", p.why);
    std::vector<float> packed(p.packed_floats, 0.0f);
    ENTER_DEVICE(c);
    HIP_TRY(hipDeviceSynchronize());         // a launch in flight may still use the fit this call replaces
    c->hf.C = 0;
    HIP_TRY(c->hf.d_m.upload(packed));
    HIP_TRY(c->hf.d_v.upload(packed));
    if (w0_host) csp_pack_head(csp_head_plan(F, C, C, 1, CSP_HEAD_PROBS), w0_host, packed.data());
    HIP_TRY(c->hf.d_w.upload(packed));
    c->hf.C = C;
    c->hf.F = F;
    c->hf.steps = 0;
    return RANGE_OK;
}

int32_t range_headfit_classes(const range_ctx* c) { return c ? c->hf.C : 0; }
int32_t range_headfit_width(const range_ctx* c) { return c && c->hf.C ? c->hf.F : 0; }
int64_t range_headfit_steps(const range_ctx* c) { return c && c->hf.C ? c->hf.steps : 0; }

int range_headfit_step_grid(range_ctx* c, const float* feats, int64_t N, const int32_t* rows, const int32_t* labels, int32_t B,
                            const float* bg, int32_t Bg, double rand_sample_weight, double lr, double beta1, double beta2,
                            double eps, double weight_decay, float* loss3, int64_t max_grid, int32_t panel_cols,
                            range_stream_t stream) {
    const HeadfitAdam adam{lr, beta1, beta2, eps, weight_decay};
    return headfit_run(c, HEADFIT_STEP, feats, N, rows, labels, B, bg, Bg, rand_sample_weight, &adam, nullptr, loss3, max_grid,
                       panel_cols, stream);
}

int range_headfit_step(range_ctx* c, const float* feats, int64_t N, const int32_t* rows, const int32_t* labels, int32_t B,
                       const float* bg, int32_t Bg, double rand_sample_weight, double lr, double beta1, double beta2, double eps,
                       double weight_decay, float* loss3, range_stream_t stream) {
    return range_headfit_step_grid(c, feats, N, rows, labels, B, bg, Bg, rand_sample_weight, lr, beta1, beta2, eps, weight_decay,
                                   loss3, 0, 0, stream);
}

int range_headfit_grad_grid(range_ctx* c, const float* feats, int64_t N, const int32_t* rows, const int32_t* labels, int32_t B,
                            const float* bg, int32_t Bg, double rand_sample_weight, float* dW, float* loss3, int64_t max_grid,
                            int32_t panel_cols, range_stream_t stream) {
    return headfit_run(c, HEADFIT_GRAD, feats, N, rows, labels, B, bg, Bg, rand_sample_weight, nullptr, dW, loss3, max_grid,
                       panel_cols, stream);
}

int range_headfit_grad(range_ctx* c, const float* feats, int64_t N, const int32_t* rows, const int32_t* labels, int32_t B,
                       const float* bg, int32_t Bg, double rand_sample_weight, float* dW, float* loss3, range_stream_t stream) {
    return range_headfit_grad_grid(c, feats, N, rows, labels, B, bg, Bg, rand_sample_weight, dW, loss3, 0, 0, stream);
}

int range_headfit_loss_grid(range_ctx* c, const float* feats, int64_t N, const int32_t* rows, const int32_t* labels, int32_t B,
                            const float* bg, int32_t Bg, double rand_sample_weight, float* loss3, int64_t max_grid,
                            int32_t panel_cols, range_stream_t stream) {
    return headfit_run(c, HEADFIT_LOSS, feats, N, rows, labels, B, bg, Bg, rand_sample_weight, nullptr, nullptr, loss3, max_grid,
                       panel_cols, stream);
}

int range_headfit_loss(range_ctx* c, const float* feats, int64_t N, const int32_t* rows, const int32_t* labels, int32_t B,
                       const float* bg, int32_t Bg, double rand_sample_weight, float* loss3, range_stream_t stream) {
    return range_headfit_loss_grid(c, feats, N, rows, labels, B, bg, Bg, rand_sample_weight, loss3, 0, 0, stream);
}

int range_headfit_weights(range_ctx* c, float* W, range_stream_t stream) {
    if (!c || !W) return fail(RANGE_ERR_INVALID, "null argument");
    if (!c->hf.C) return fail(RANGE_ERR_STATE, "no class-head fit begun (range_headfit_begin)");
    if (!aligned(W, 4)) return fail(RANGE_ERR_INVALID, "the device pointer must be 4-byte aligned");
    const HeadfitPlan p = headfit_plan(c->hf.C, c->hf.F, 1);
    ENTER_DEVICE(c);
    return launch(headfit_unpack_kernel, dim3(p.unpack_grid), dim3(p.block), 0, (hipStream_t)stream, (const float*)c->hf.d_w.p,
                  (int32_t)c->hf.C, (int32_t)c->hf.F, (int32_t)p.k_groups, W);
}

}  // extern "C"
