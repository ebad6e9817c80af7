// Host side of the bank: range_set_bank, range_set_keys, range_set_pv_mode - the uploads, the fragment copies of the
// keys, the norms the softmax kernels rely on, the bf16 planes of the values.  Part of range_hip.hip's translation unit.
#pragma once

// the three bf16 planes of the bank's values in MFMA fragment order (attend_bf16x3.h); 6 B per value
static int build_vplanes(range_ctx* c) {
    const int64_t n_groups = (c->bank.n_rows + 31) / 32;
    if (c->bank.d_vplanes.ensure((size_t)n_groups * (PVB_GROUP_BYTES / 4)) != hipSuccess)
        return fail(RANGE_ERR_NOMEM, "out of device memory for the bf16 planes of the values (%lld MB)",
                    (long long)(n_groups * PVB_GROUP_BYTES >> 20));
    const int64_t threads = n_groups * 64 * 64;
    if (int lrc = launch(vplanes_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, 0, c->bank.d_values.p,
                       c->bank.n_pad, n_groups, reinterpret_cast<u32x4*>(c->bank.d_vplanes.p))) return lrc;
    HIP_TRY(hipDeviceSynchronize());
    c->bank.vplanes_groups = n_groups;
    return RANGE_OK;
}

// keys -> device (float32 rows + the bf16 fragment copy the prefilter of range_topk_stream
// streams) and the largest row norm, computed on the device.  `keys` may be a host or a device
// pointer (hipMemcpyDefault).
static int upload_keys(range_ctx* c, const float* keys, int64_t n_rows, int64_t n_pad) {
    c->bank.tg_key_scale = 0.f;       // (the batch top-k rebuilds its fp16 copy for the new keys)
    HIP_TRY(c->bank.d_keys.ensure((size_t)n_pad * KEY_DIM));
    if (n_pad > n_rows)
        HIP_TRY(hipMemset(c->bank.d_keys.p + (size_t)n_rows * KEY_DIM, 0, (size_t)(n_pad - n_rows) * KEY_DIM * 4));
    HIP_TRY(hipMemcpy(c->bank.d_keys.p, keys, (size_t)n_rows * KEY_DIM * 4, hipMemcpyDefault));
    const int64_t n_tiles = n_pad / BLK;
    HIP_TRY(c->bank.d_keys_bf16.ensure((size_t)n_tiles * (TSB_TILE_BYTES / 4)));
    const int64_t threads = n_tiles * 8 * 64;
    if (int lrc = launch(keyfrag_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, 0, c->bank.d_keys.p,
                       n_pad, n_tiles, reinterpret_cast<u32x4*>(c->bank.d_keys_bf16.p))) return lrc;
    if (!c->topk.ws_topk_sync.p) {
        HIP_TRY(c->topk.ws_topk_sync.ensure(TOPKS_SYNC_WORDS));
        HIP_TRY(hipMemset(c->topk.ws_topk_sync.p, 0, TOPKS_SYNC_WORDS * 4));
        std::memset(c->topk.topk_sync_base, 0, sizeof c->topk.topk_sync_base);
    }
    uint32_t* scratch = c->topk.ws_topk_sync.p + TOPKS_SYNC_SCRATCH;
    HIP_TRY(hipMemset(scratch, 0, 4));
    if (int lrc = launch(key_norm_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, 0, c->bank.d_keys.p, n_rows, scratch)) return lrc;
    float n2max = 0.f;
    HIP_TRY(hipMemcpy(&n2max, scratch, 4, hipMemcpyDeviceToHost));   // (synchronises)
    // (a bound: the float32 sum of squares is within 3e-5 of the exact one)
    c->bank.key_norm_max = (float)(std::sqrt((double)n2max) * 1.0001);
    return RANGE_OK;
}

// The bank of range_set_bank, or - values and xyz null - the keys-only bank of range_set_keys:
// argument checks, padding to whole blocks, the state a new bank resets, uploads, commit.
static int commit_bank(range_ctx* c, const float* keys, const float* values, const float* xyz,
                       int64_t n_rows, int64_t row_offset) {
    if (n_rows <= 0) return fail(RANGE_ERR_INVALID, "n_rows must be > 0");
    if (n_rows >= (int64_t)1 << 31) return fail(RANGE_ERR_INVALID, "n_rows too large");
    ENTER_DEVICE(c);
    const int64_t n_pad = (n_rows + BLK - 1) / BLK * BLK;
    c->bank.has_bank = false;
    c->bank.has_values = false;
    c->kept.kept_B = 0;
    if (values) {
        HIP_TRY(c->bank.d_values.ensure((size_t)n_pad * VAL_DIM));
        HIP_TRY(c->bank.d_xyz4.ensure((size_t)n_pad * 4));
        HIP_TRY(hipMemset(c->bank.d_values.p, 0, (size_t)n_pad * VAL_DIM * 4));
        HIP_TRY(hipMemset(c->bank.d_xyz4.p, 0, (size_t)n_pad * 16));
        HIP_TRY(hipMemcpy(c->bank.d_values.p, values, (size_t)n_rows * VAL_DIM * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy2D(c->bank.d_xyz4.p, 16, xyz, 12, 12, (size_t)n_rows, hipMemcpyHostToDevice));
        double n2max = 0.0;
        for (int64_t r = 0; r < n_rows; ++r) {
            const float* x = xyz + 3 * r;
            n2max = std::max(n2max, (double)x[0] * x[0] + (double)x[1] * x[1] + (double)x[2] * x[2]);
        }
        c->bank.xyz_norm_max = (float)std::sqrt(n2max);
    } else {
        c->bank.d_values.release();
        c->bank.d_xyz4.release();
        c->bank.d_vplanes.release();
    }
    if (int lrc = upload_keys(c, keys, n_rows, n_pad)) return lrc;
    HIP_TRY(hipDeviceSynchronize());
    c->bank.n_rows = n_rows;
    c->bank.n_pad = n_pad;
    c->bank.row_offset = row_offset;
    c->bank.has_bank = true;
    c->bank.has_values = values != nullptr;
    c->bank.vplanes_groups = 0;
    if (values && c->bank.pv_mode == RANGE_PV_BF16X3) return build_vplanes(c);
    return RANGE_OK;
}

extern "C" {

int64_t range_bank_rows(const range_ctx* ctx) { return ctx ? ctx->bank.n_rows : 0; }

int range_set_bank(range_ctx* c, const float* keys, const float* values, const float* xyz,
                   int64_t n_rows, int64_t row_offset) {
    if (!c || !keys || !values || !xyz) return fail(RANGE_ERR_INVALID, "null argument");
    return commit_bank(c, keys, values, xyz, n_rows, row_offset);
}

int range_set_keys(range_ctx* c, const float* keys, int64_t n_rows, int64_t row_offset) {
    if (!c || !keys) return fail(RANGE_ERR_INVALID, "null argument");
    return commit_bank(c, keys, nullptr, nullptr, n_rows, row_offset);
}

int range_set_pv_mode(range_ctx* c, int32_t mode) {
    if (!c) return fail(RANGE_ERR_INVALID, "null argument");
    if (mode != RANGE_PV_EXACT && mode != RANGE_PV_BF16X3) return fail(RANGE_ERR_INVALID, "unknown pv mode %d", mode);
    ENTER_DEVICE(c);
    c->bank.pv_mode = mode;
    // (a keys-only bank has no values to split: the next range_set_bank builds the planes)
    if (mode == RANGE_PV_BF16X3 && c->bank.has_bank && c->bank.has_values && c->bank.vplanes_groups == 0) return build_vplanes(c);
    return RANGE_OK;
}
int32_t range_get_pv_mode(const range_ctx* c) { return c ? c->bank.pv_mode : -1; }

}  // extern "C"
