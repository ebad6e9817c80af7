// Host side of the positional encoders (posenc_kernel.h): range_posenc_width, range_posenc_features.
// Part of range_hip.hip's translation unit, behind engine_ctx.h.
#pragma once

// the positional encoders, by kind
static void (*posenc_kernel_for(int kind))(PosencArgs) {
    static void (*const posenc_kernels[PE_KINDS])(PosencArgs) = {
        posenc_features_kernel<PE_THEORY>, posenc_features_kernel<PE_GRID>, posenc_features_kernel<PE_SPHEREC>,
        posenc_features_kernel<PE_SPHERECPLUS>, posenc_features_kernel<PE_SPHEREM>, posenc_features_kernel<PE_SPHEREMPLUS>};
    return posenc_kernels[kind];
}

// The device copy of a frequency table: the context keeps every table it has seen (a model has one; at
// most POSENC_TABLES_MAX, beyond which the device is drained and the tables are dropped).  A new table
// costs one allocation and a synchronous upload; a known one nothing.
constexpr size_t POSENC_TABLES_MAX = 64;
static int posenc_table(range_ctx* c, const double* freq_host, int32_t F, const double** dev) {
    auto& tables = c->posenc.tables;
    for (auto& t : tables)
        if ((int32_t)t->host.size() == F && std::memcmp(t->host.data(), freq_host, (size_t)F * sizeof(double)) == 0) {
            *dev = t->dev.p;
            return RANGE_OK;
        }
    if (tables.size() >= POSENC_TABLES_MAX) {
        HIP_TRY(hipDeviceSynchronize());
        tables.clear();
    }
    auto t = std::make_unique<range_ctx::Posenc::Table>();
    t->host.assign(freq_host, freq_host + F);
    HIP_TRY(t->dev.upload(t->host));
    *dev = t->dev.p;
    tables.push_back(std::move(t));
    return RANGE_OK;
}

extern "C" {

int32_t range_posenc_width(int32_t kind, int32_t F) {
    if (F < 1 || F > POSENC_MAX_F) return 0;
    return posenc_per_freq(kind) * F;
}

int range_posenc_features(range_ctx* c, int32_t kind, const double* freq_host, int32_t F, const double* lonlat,
                          int64_t B, double* out, range_stream_t stream) {
    if (!c || !freq_host || !lonlat || !out) return fail(RANGE_ERR_INVALID, "null argument");
    if (kind < 0 || kind >= PE_KINDS) return fail(RANGE_ERR_INVALID, "positional encoder kind %d", kind);
    if (F < 1 || F > POSENC_MAX_F) return fail(RANGE_ERR_INVALID, "F = %d frequencies (1 .. %d)", F, POSENC_MAX_F);
    if (B <= 0) return fail(RANGE_ERR_INVALID, "B must be > 0");
    if (!aligned(out, 16)) return fail(RANGE_ERR_INVALID, "out_dev must be 16-byte aligned");
    const PosencPlan p = posenc_plan(kind, F, B);
    if (!p.valid) return fail(RANGE_ERR_INVALID, "B = %lld locations: output too large", (long long)B);
    ENTER_DEVICE(c);
    PosencArgs a{};
    if (int rc = posenc_table(c, freq_host, F, &a.freq)) return rc;
    a.lonlat = lonlat;
    a.out = out;
    a.B = B;
    a.n_tiles = p.n_tiles;
    a.F = F;
    return launch(posenc_kernel_for(kind), dim3(p.grid), dim3(p.block), p.lds_bytes, (hipStream_t)stream, a);
}

}  // extern "C"
