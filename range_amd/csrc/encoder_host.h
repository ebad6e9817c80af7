// Host side of the location encoder (encoder_kernel.h) and the training-free coordinate encoders: range_set_encoder,
// range_set_sh_table, range_encode, range_encode_raw, range_coord_features; encode_to_workspace for the forward
// calls.  Part of range_hip.hip's translation unit.
#pragma once

// The encoder kernels are instantiated per width in 64-column tiles (of the hidden layer, or of a
// column part of it): the variants that exist, with the waves of their workgroups.
struct EncVariant { int nt; void (*kernel)(EncArgs); int waves; };
// waves per encoder workgroup when the hidden width is a multiple of 256 (4 or 16)
constexpr int ENC_WAVES = 16;
const EncVariant ENC_TILE[] = {
    {1, encoder_tile_kernel<1, 4>, ENC_PART_WAVES}, {2, encoder_tile_kernel<2, 8>, ENC_PART_WAVES},
    {4, encoder_tile_kernel<4, 8>, ENC_PART_WAVES}, {8, encoder_tile_kernel<8, 16>, ENC_PART_WAVES}};
const EncVariant ENC_L1_PART[] = {
    {1, encoder_l1_part_kernel<1, 4>, ENC_PART_WAVES}, {2, encoder_l1_part_kernel<2, 8>, ENC_PART_WAVES},
    {4, encoder_l1_part_kernel<4, 8>, ENC_PART_WAVES}, {8, encoder_l1_part_kernel<8, 16>, ENC_PART_WAVES}};
const EncVariant ENC_L2_PART[] = {
    {1, encoder_l2_part_kernel<1>, 4}, {2, encoder_l2_part_kernel<2>, 8}, {4, encoder_l2_part_kernel<4>, 16}};
const EncVariant ENC_REST[] = {
    {1, encoder_rest_kernel<1, 4>, 4}, {2, encoder_rest_kernel<2, 4>, 4}, {4, encoder_rest_kernel<4, ENC_WAVES>, ENC_WAVES},
    {6, encoder_rest_kernel<6, 4>, 4}, {8, encoder_rest_kernel<8, ENC_WAVES>, ENC_WAVES},
    {12, encoder_rest_kernel<12, 16>, 16}, {16, encoder_rest_kernel<16, 16>, 16}};
// 16 waves per workgroup where the hidden width allows (multiples of 256), else 4
const EncVariant ENC_MAIN[] = {
    {1, encoder_kernel<1, 4>, 4}, {2, encoder_kernel<2, 4>, 4}, {3, encoder_kernel<3, 4>, 4},
    {4, encoder_kernel<4, ENC_WAVES>, ENC_WAVES}, {5, encoder_kernel<5, 4>, 4}, {6, encoder_kernel<6, 4>, 4},
    {7, encoder_kernel<7, 4>, 4}, {8, encoder_kernel<8, ENC_WAVES>, ENC_WAVES}, {12, encoder_kernel<12, 16>, 16},
    {16, encoder_kernel<16, 16>, 16}};

template <size_t N>
static int launch_encoder_variant(const EncVariant (&table)[N], int cols, const char* no_variant, int grid, size_t lds,
                                  hipStream_t s, const EncArgs& a) {
    for (const EncVariant& v : table)
        if (v.nt == cols / 64) return launch(v.kernel, dim3(grid), dim3(v.waves * 64), lds, s, a);
    return fail(RANGE_ERR_INVALID, no_variant, cols);
}

// the small-batch kernels on the queries of `a`, as host_plan.h: plan_encoder_split lays them out
static int launch_encoder_split(range_ctx* c, EncArgs a, const EncSplitPlan& sp, hipStream_t s) {
    if (c->enc.ws_h1.ensure(sp.h1_doubles) != hipSuccess) return fail(RANGE_ERR_NOMEM, "out of device memory");
    a.h1 = c->enc.ws_h1.p;
    a.n_parts = sp.S;
    a.part_cols = sp.part_cols;
    a.n_kparts = sp.KP;
    a.n_wg32 = 0;
    a.n_parts2 = sp.n_parts2;      // (read by the second-layer phase / launch and the last one only)
    a.part2_cols = sp.part2_cols;
    a.rest_from = sp.rest_from;
    const size_t lds = c->enc.lds_bytes;
    ProfScope ps(c, RANGE_PROF_ENCODER, s);
    if (sp.one_launch) {
        if (c->enc.ws_h2.ensure(sp.tile_doubles) != hipSuccess || c->enc.ws_h1a.ensure(sp.tile_doubles) != hipSuccess ||
            c->enc.ws_e3.ensure((size_t)sp.tiles * 16 * ENC_EMBED) != hipSuccess || c->enc.ws_enc_sync.ensure(128 * 256) != hipSuccess)
            return fail(RANGE_ERR_NOMEM, "out of device memory");
        // (the counters wrap to zero by themselves, but a launch whose bounded spin gave up would leave
        // them poisoned for good: zeroed in front of every launch - 2 us of a ~55 us kernel - as the
        // guide asks of every polled word)
        HIP_TRY(hipMemsetAsync(c->enc.ws_enc_sync.p, 0, (size_t)sp.tiles * 256 * 4, s));
        a.h2 = c->enc.ws_h2.p;
        a.h1a = c->enc.ws_h1a.p;
        a.e3 = c->enc.ws_e3.p;
        a.sync = c->enc.ws_enc_sync.p;
        a.err = c->d_async_err ? c->d_async_err + RANGE_ASYNC_WORD_ENCODER : nullptr;
        a.debug_giveup = c->debug_giveup_next ? 1 : 0;
        c->debug_giveup_next = false;
        return launch_encoder_variant(ENC_TILE, sp.part_cols, "internal: encoder part width %d", sp.grid, lds, s, a);
    }
    if (int rc = launch_encoder_variant(ENC_L1_PART, sp.part_cols, "internal: encoder part width %d", sp.grid, lds, s, a)) return rc;
    if (sp.S2 > 1) {
        if (c->enc.ws_h2.ensure(sp.tile_doubles) != hipSuccess) return fail(RANGE_ERR_NOMEM, "out of device memory");
        a.h2 = c->enc.ws_h2.p;
        if (int rc = launch_encoder_variant(ENC_L2_PART, sp.part2_cols, "internal: encoder part width %d", sp.tiles * sp.S2, lds, s, a)) return rc;
    }
    return launch_encoder_variant(ENC_REST, a.H, "internal: hidden width %d", sp.tiles, lds, s, a);
}

static int launch_encoder(range_ctx* c, const EncArgs& a_in, hipStream_t s) {
    const EncLaunchPlan p = plan_encoder(c->n_cu, a_in.n_slots, a_in.H, a_in.n_layers, c->sw.enc_split, c->sw.enc_fused,
                                         a_in.B, ENC_QTILE);
    if (p.main_B > 0) {
        EncArgs a = a_in;
        a.B = p.main_B;
        a.n_wg32 = p.n_wg32;
        ProfScope ps(c, RANGE_PROF_ENCODER, s);
        if (int rc = launch_encoder_variant(ENC_MAIN, a.H, "unsupported hidden width %d", p.grid, c->enc.lds_bytes, s, a)) return rc;
    }
    if (p.split_B > 0) {
        // the queries behind the main launch
        const int64_t b_main = p.main_B;
        EncArgs t = a_in;
        t.B = p.split_B;
        t.lonlat = a_in.lonlat + 2 * b_main;
        t.ehat64 = a_in.ehat64 + ENC_EMBED * b_main;
        t.eraw64 = a_in.eraw64 ? a_in.eraw64 + ENC_EMBED * b_main : nullptr;
        t.ehat32 = a_in.ehat32 + ENC_EMBED * b_main;
        t.xq = a_in.xq + 4 * b_main;
        return launch_encoder_split(c, t, p.split, s);
    }
    return RANGE_OK;
}

static int encode_impl(range_ctx* c, const double* lonlat, int64_t B, double* ehat64, float* ehat32,
                       float* xq32, double* eraw64, range_stream_t stream) {
    if (!c || !lonlat || !ehat64 || !ehat32 || !xq32) return fail(RANGE_ERR_INVALID, "null argument");
    if (!c->enc.has_encoder) return fail(RANGE_ERR_STATE, "encoder not set (range_set_encoder)");
    if (B <= 0) return fail(RANGE_ERR_INVALID, "B must be > 0");
    if (int rc = check_async_error(c)) return rc;
    ENTER_DEVICE(c);
    EncArgs a = c->enc.args;
    a.lonlat = lonlat;
    a.ehat64 = ehat64;
    a.eraw64 = eraw64;
    a.ehat32 = ehat32;
    a.xq = xq32;
    a.B = B;
    return launch_encoder(c, a, (hipStream_t)stream);
}

// The context's query workspace (e-hat in both precisions, xq, the softmax statistics) sized for B
// queries, and the encoder into it; eraw64: the un-normalised outputs too, or null.
static int encode_to_workspace(range_ctx* c, const double* lonlat, int64_t B, double* eraw64, range_stream_t stream) {
    if (B <= 0) return fail(RANGE_ERR_INVALID, "B must be > 0");
    ENTER_DEVICE(c);
    HIP_TRY(c->pass.ws_ehat64.ensure((size_t)B * 256));
    HIP_TRY(c->pass.ws_ehat32.ensure((size_t)B * 256));
    HIP_TRY(c->pass.ws_xq.ensure((size_t)B * 4));
    HIP_TRY(c->pass.ws_stats.ensure((size_t)B * 4));
    return encode_impl(c, lonlat, B, c->pass.ws_ehat64.p, c->pass.ws_ehat32.p, c->pass.ws_xq.p, eraw64, stream);
}

extern "C" {

int range_set_encoder(range_ctx* c, const range_encoder_desc* d, const double* const* weights,
                      const double* const* biases) {
    if (!c || !d || !weights || !biases) return fail(RANGE_ERR_INVALID, "null argument");
    const int L = d->legendre_polys, Hc = d->hidden, NL = d->num_hidden_layers, E = d->embed_dim;
    if (L < 1 || L > 64) return fail(RANGE_ERR_INVALID, "legendre_polys %d unsupported (1..64)", L);
    // (`capacity` of the real checkpoint is unknown: a width no kernel exists for runs zero-padded as
    // the next one that has - host_plan.h: kernel_hidden_width - at the padded width's cost)
    const int H = kernel_hidden_width(Hc);
    if (H == 0) return fail(RANGE_ERR_INVALID, "hidden %d unsupported (1..1024)", Hc);
    if (NL < 1 || NL + 1 > ENC_MAX_LAYERS) return fail(RANGE_ERR_INVALID, "num_hidden_layers %d unsupported", NL);
    if (E != ENC_EMBED) return fail(RANGE_ERR_INVALID, "embed_dim %d unsupported (must be 256)", E);
    if (d->sh_mode != RANGE_SH_ANALYTIC && d->sh_mode != RANGE_SH_CLOSED_FORM)
        return fail(RANGE_ERR_INVALID, "unknown sh_mode %d", d->sh_mode);
    ENTER_DEVICE(c);

    // ---- slot plan, recurrence tables, weight packing: pure host arithmetic (host_plan.h, also
    //      built and run under sanitizers on the CPU: tests/native/host_sanitize.cpp)
    EncoderPlan plan;
    if (!build_encoder_plan(L, ENC_SLOTS_PER_ROUND, plan)) return fail(RANGE_ERR_INVALID, "internal: slot plan is not a permutation");
    const int n_slots = plan.n_slots, n_rounds = plan.n_rounds, Kp = (int)plan.perm.size();
    // (hidden widths beyond 512 run 16-query workgroups only, their activations packed densely)
    const int lds_main = (H > 512 ? 16 : ENC_QTILE) * std::max(plan.max_round, H);
    const size_t lds_bytes = (size_t)(lds_main + 16 * ENC_QTILE) * sizeof(double);   // + [<= 16 waves][32] partial norms
    if (lds_bytes > 160 * 1024) return fail(RANGE_ERR_INVALID, "encoder shape needs %zu B of LDS (>160 KiB)", lds_bytes);
    std::vector<double> coefA, coefB, seedc;
    recurrence_tables(L, d->sh_mode == RANGE_SH_ANALYTIC, coefA, coefB, seedc);
    for (int i = 0; i <= NL; ++i) if (!weights[i] || !biases[i]) return fail(RANGE_ERR_INVALID, "weights[%d]/biases[%d] null", i, i);
    // (H == Hc: the padding is a plain copy)
    HIP_TRY(c->enc.d_wp[0].upload(pack_weights(pad_weights(weights[0], Hc, L * L, H, L * L).data(), H, L * L, &plan.perm, Kp)));
    for (int i = 1; i < NL; ++i) HIP_TRY(c->enc.d_wp[i].upload(pack_weights(pad_weights(weights[i], Hc, Hc, H, H).data(), H, H, nullptr, H)));
    HIP_TRY(c->enc.d_wp[NL].upload(pack_weights(pad_weights(weights[NL], E, Hc, E, H).data(), E, H, nullptr, H)));
    for (int i = 0; i <= NL; ++i) {
        std::vector<double> b((size_t)(i < NL ? H : E), 0.0);
        std::copy(biases[i], biases[i] + (i < NL ? Hc : E), b.begin());
        HIP_TRY(c->enc.d_bias[i].upload(b));
    }
    HIP_TRY(c->enc.d_slot_base.upload(plan.slot_base));
    HIP_TRY(c->enc.d_coefA.upload(coefA));
    HIP_TRY(c->enc.d_coefB.upload(coefB));
    HIP_TRY(c->enc.d_seedc.upload(seedc));

    EncArgs& a = c->enc.args;
    a = EncArgs{};
    a.L = L;
    a.n_slots = n_slots;
    a.n_rounds = n_rounds;
    a.n_layers = NL;
    a.H = H;
    a.kp0_total = Kp / 8;
    a.lds_main_doubles = lds_main;
    a.slot_base = c->enc.d_slot_base.p;
    a.coefA = c->enc.d_coefA.p;
    a.coefB = c->enc.d_coefB.p;
    a.seedc = c->enc.d_seedc.p;
    for (int i = 0; i <= NL; ++i) { a.wp[i] = c->enc.d_wp[i].p; a.bias[i] = c->enc.d_bias[i].p; }
    c->enc.lds_bytes = c->enc.lds_base = lds_bytes;
    c->enc.desc = *d;
    c->enc.has_encoder = true;
    return RANGE_OK;
}

int range_set_sh_table(range_ctx* c, int32_t L, const double* front, const double* a0, const double* a2,
                       const int32_t* p2, const int32_t* kx, const int32_t* off, const int32_t* cnt,
                       int64_t n_terms, const double* coef, const int32_t* pw) {
    if (!c || !front || !a0 || !a2 || !p2 || !kx || !off || !cnt || (n_terms > 0 && (!coef || !pw)))
        return fail(RANGE_ERR_INVALID, "null argument");
    if (!c->enc.has_encoder) return fail(RANGE_ERR_STATE, "encoder not set (range_set_encoder)");
    if (c->enc.desc.sh_mode != RANGE_SH_ANALYTIC)
        return fail(RANGE_ERR_INVALID, "the coefficient table belongs to the 'analytic' spherical harmonics");
    if (L != c->enc.desc.legendre_polys) return fail(RANGE_ERR_INVALID, "table for L=%d, encoder has L=%d", L, c->enc.desc.legendre_polys);
    ENTER_DEVICE(c);
    std::vector<SHDesc> desc((size_t)L * L);
    for (int l = 0; l < L; ++l)
        for (int m = 0; m <= l; ++m) {
            const int i = l * L + m;
            if (cnt[i] < 0 || off[i] < 0 || (int64_t)off[i] + cnt[i] > n_terms || p2[i] < 0 || p2[i] > 127 ||
                kx[i] < 0 || kx[i] >= L || cnt[i] > 32767)
                return fail(RANGE_ERR_INVALID, "bad table entry (l=%d, m=%d)", l, m);
            desc[i] = SHDesc{front[i], a0[i], a2[i], off[i], (int16_t)cnt[i], (int8_t)p2[i], (int8_t)kx[i]};
        }
    for (int64_t j = 0; j < n_terms; ++j)
        if (pw[j] < 0 || pw[j] >= L) return fail(RANGE_ERR_INVALID, "power %d out of range at term %lld", pw[j], (long long)j);
    const size_t lds = c->enc.lds_base + (size_t)ENC_QTILE * L * sizeof(double);
    if (lds > 160 * 1024) return fail(RANGE_ERR_INVALID, "encoder shape needs %zu B of LDS with the power table (>160 KiB)", lds);
    HIP_TRY(c->enc.d_sh_desc.upload(desc));
    // (L <= 2: every function is a monomial and there are no terms - upload one zero, read nothing)
    HIP_TRY(c->enc.d_sh_coef.upload(n_terms > 0 ? std::vector<double>(coef, coef + n_terms) : std::vector<double>(1, 0.0)));
    HIP_TRY(c->enc.d_sh_pow.upload(n_terms > 0 ? std::vector<int32_t>(pw, pw + n_terms) : std::vector<int32_t>(1, 0)));
    c->enc.args.sh_desc = c->enc.d_sh_desc.p;
    c->enc.args.sh_coef = c->enc.d_sh_coef.p;
    c->enc.args.sh_pow = c->enc.d_sh_pow.p;
    c->enc.lds_bytes = lds;
    return RANGE_OK;
}

int range_encode(range_ctx* c, const double* lonlat, int64_t B, double* ehat64, float* ehat32,
                 float* xq32, range_stream_t stream) {
    return encode_impl(c, lonlat, B, ehat64, ehat32, xq32, nullptr, stream);
}

int range_encode_raw(range_ctx* c, const double* lonlat, int64_t B, double* eraw64,
                     range_stream_t stream) {
    if (!c || !eraw64) return fail(RANGE_ERR_INVALID, "null argument");
    const int rc = encode_to_workspace(c, lonlat, B, eraw64, stream);
    c->pass.ws_queries = rc == RANGE_OK ? B : 0;
    return rc;
}

int range_coord_features(range_ctx* c, int32_t mode, const double* lonlat, int64_t B, double* out,
                         range_stream_t stream) {
    if (!c || !lonlat || !out) return fail(RANGE_ERR_INVALID, "null argument");
    if (mode < 0 || mode > 2) return fail(RANGE_ERR_INVALID, "coordinate encoder mode %d", mode);
    if (B <= 0) return fail(RANGE_ERR_INVALID, "B must be > 0");
    ENTER_DEVICE(c);
    return launch(coord_features_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, mode, lonlat, B, out);
}

}  // extern "C"
