// librange_hip.so - C ABI (include/range_hip.h) over the hand-written gfx950 kernels.
// Host side of the engine: context, one-time weight/bank packing, launch geometry, workspace.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/range_hip.h"
#include "host_common.h"
#include "host_copy.h"
#include "host_plan.h"
#include "scan_common.h"
#include "topk_lists.h"
#include "pass1.h"
#include "pass1_sharp.h"
#include "pass1_kept.h"
#include "pass2.h"
#include "topk_stream.h"
#include "topk_gemm.h"
#include "attend_bf16x3.h"
#include "attend_small.h"
#include "encoder_kernel.h"
#include "posenc_kernel.h"
#include "csp_kernel.h"
#include "csp_head_kernel.h"
#include "csp_rank_kernel.h"
#include "checker_kernel.h"
#include "neighbor_kernel.h"

using namespace range_hip;
using namespace range_host;

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
    // chunks' partial count rows of a split scan, the selection of a k-nearest-neighbour call
    struct Neighbors {
        int64_t N = 0;                   // 0: no set installed
        int C = 0;
        bool hav = false, has_cells = false;
        DevBuf<NeighborPoint> d_pts;
        DevBuf<int32_t> ws_counts;
        DevBuf<double> ws_redk;
        DevBuf<int64_t> ws_jlast;
    } nb;
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

// The encoder kernels are instantiated per width in 64-column tiles (of the hidden layer, or of a
// column part of it): the variants that exist, with the waves of their workgroups.  (The kernel tables
// of this file keep the order of first use: hipcc emits the instantiations, and numbers their labels, in it.)
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
int launch_encoder_variant(const EncVariant (&table)[N], int cols, const char* no_variant, int grid, size_t lds,
                           hipStream_t s, const EncArgs& a) {
    for (const EncVariant& v : table)
        if (v.nt == cols / 64) return launch(v.kernel, dim3(grid), dim3(v.waves * 64), lds, s, a);
    return fail(RANGE_ERR_INVALID, no_variant, cols);
}

// the small-batch kernels on the queries of `a`, as host_plan.h: plan_encoder_split lays them out
int launch_encoder_split(range_ctx* c, EncArgs a, const EncSplitPlan& sp, hipStream_t s) {
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

int launch_encoder(range_ctx* c, const EncArgs& a_in, hipStream_t s) {
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

// the three bf16 planes of the bank's values in MFMA fragment order (attend_bf16x3.h); 6 B per value
int build_vplanes(range_ctx* c) {
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

static_assert(MAX_TAU_CONSTANT == RANGE_MAX_TAU && MAX_TAU_SHARP == RANGE_MAX_TAU_SHARP, "host_plan.h and range_hip.h disagree");

// Preconditions and scales of every kernel that forms softmax weights: k_sem / k_geo are the
// temperatures in the kernels' base-2 form (k_geo 0: no geographic head).  max_tau: the cap that fits
// the caller - RANGE_MAX_TAU for a kernel with the constant shift m = tau * log2(e), RANGE_MAX_TAU_SHARP
// for one that takes its shift from the statistics (pass 2) or keeps a running maximum.
int softmax_scales(range_ctx* c, int64_t B, float tau_sem, float tau_geo, float max_tau, float& k_sem, float& k_geo) {
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
int fill_scan_args(range_ctx* c, ScanArgs& a, const float* ehat32, const float* xq, int64_t B,
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

extern "C" {

int range_abi_version(void) { return RANGE_ABI_VERSION; }
const char* range_last_error(void) { return g_err.c_str(); }
#ifndef RANGE_BUILD_FLAGS
#define RANGE_BUILD_FLAGS ""
#endif
const char* range_build_flags(void) { return RANGE_BUILD_FLAGS; }
#ifndef RANGE_SRC_SHA256
#define RANGE_SRC_SHA256 "unknown"
#endif
// (the literal is also what range_amd/_srchash.py: library_stamp() finds in the file without loading it)
static const char g_src_stamp[] = "RANGE_SRC_SHA256=" RANGE_SRC_SHA256;
const char* range_source_sha256(void) { return g_src_stamp + 17; }

int range_create(int device, range_ctx** out) {
    if (!out) return fail(RANGE_ERR_INVALID, "out is null");
    *out = nullptr;
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count));
    if (device < 0 || device >= count)
        return fail(RANGE_ERR_INVALID, "device %d out of range (%d visible)", device, count);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(RANGE_ERR_INVALID, "device %d is %s; this library is built for gfx950 only",
                    device, prop.gcnArchName);
    range_ctx* c = new (std::nothrow) range_ctx();
    if (!c) return fail(RANGE_ERR_NOMEM, "out of host memory");
    c->device = device;
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    c->sw = parse_switches();
    {
        DeviceGuard g(device);
        void* hp = nullptr;
        void* dp = nullptr;
        if (hipHostMalloc(&hp, 64, hipHostMallocMapped) == hipSuccess) {
            std::memset(hp, 0, 64);
            if (hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess) {
                c->h_async_err = (uint32_t*)hp;
                c->d_async_err = (uint32_t*)dp;
            } else {
                (void)hipHostFree(hp);
            }
        }
        (void)hipGetLastError();       // (without the word the kernels simply do not report)
    }
    *out = c;
    return RANGE_OK;
}

void range_destroy(range_ctx* ctx) {
    if (!ctx) return;
    DeviceGuard g(ctx->device);
    (void)hipDeviceSynchronize();
    delete ctx;
}

int64_t range_bank_rows(const range_ctx* ctx) { return ctx ? ctx->bank.n_rows : 0; }

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
    if (mode == RANGE_PV_BF16X3 && c->bank.has_bank && c->bank.vplanes_groups == 0) return build_vplanes(c);
    return RANGE_OK;
}
int32_t range_get_pv_mode(const range_ctx* c) { return c ? c->bank.pv_mode : -1; }

int range_set_temperatures(range_ctx* c, float tau_sem, float tau_geo) {
    if (!c) return fail(RANGE_ERR_INVALID, "null argument");
    // 0: the model's default; anything else must be a temperature the kernels take
    if ((tau_sem != 0.f && !temperature_ok(tau_sem, RANGE_MAX_TAU_SHARP)) || (tau_geo != 0.f && !temperature_ok(tau_geo, RANGE_MAX_TAU_SHARP)))
        return fail(RANGE_ERR_INVALID, "temperatures must be finite, > 0 and at most %g, or 0 for the model's default (tau_sem %g, tau_geo %g)",
                    (double)RANGE_MAX_TAU_SHARP, (double)tau_sem, (double)tau_geo);
    c->tau_sem_set = tau_sem;
    c->tau_geo_set = tau_geo;
    return RANGE_OK;
}

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

int range_check_async_error(range_ctx* c) {
    if (!c) return fail(RANGE_ERR_INVALID, "null argument");
    return check_async_error(c);
}

// test hook: the NEXT persistent launch of this context (the one-launch encoder of up to 512 queries,
// or the fused top-k) behaves as if its bounded in-launch wait had expired - the real give-up path:
// NaN / -1 outputs, the host-mapped word, the fall-back (tests/test_gpu_round2.py)
int range_debug_raise_async_error(range_ctx* c, range_stream_t) {
    if (!c) return fail(RANGE_ERR_INVALID, "null argument");
    if (!c->d_async_err) return fail(RANGE_ERR_STATE, "no host-mapped error word in this context");
    c->debug_giveup_next = true;
    return RANGE_OK;
}

// The give-up words as DATA, in stream order (range_hip.h: range_async_error_flag): a rank of a
// row-sharded job sends this with its rows, so that every rank learns from the WORD - not from NaN in
// the data, which a NaN coordinate produces as well - that a peer's persistent launch gave up.
__global__ void async_flag_kernel(const uint32_t* __restrict__ err, double* __restrict__ flag) {
    if (threadIdx.x == 0 && blockIdx.x == 0)
        flag[0] = (__hip_atomic_load(err + RANGE_ASYNC_WORD_ENCODER, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) |
                   __hip_atomic_load(err + RANGE_ASYNC_WORD_TOPK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) ? 1.0 : 0.0;
}

int range_async_error_flag(range_ctx* c, double* flag_dev, range_stream_t stream) {
    if (!c || !flag_dev) return fail(RANGE_ERR_INVALID, "null argument");
    ENTER_DEVICE(c);
    if (!c->d_async_err) {            // (no host-mapped words in this context: nothing can have been reported)
        HIP_TRY(hipMemsetAsync(flag_dev, 0, sizeof(double), (hipStream_t)stream));
        return RANGE_OK;
    }
    return launch(async_flag_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, c->d_async_err, flag_dev);
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

int range_encode(range_ctx* c, const double* lonlat, int64_t B, double* ehat64, float* ehat32,
                 float* xq32, range_stream_t stream) {
    return encode_impl(c, lonlat, B, ehat64, ehat32, xq32, nullptr, stream);
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

int range_encode_raw(range_ctx* c, const double* lonlat, int64_t B, double* eraw64,
                     range_stream_t stream) {
    if (!c || !eraw64) return fail(RANGE_ERR_INVALID, "null argument");
    const int rc = encode_to_workspace(c, lonlat, B, eraw64, stream);
    c->pass.ws_queries = rc == RANGE_OK ? B : 0;
    return rc;
}

// Training-free coordinate encoders of the reference (range/range.py:262-272): one thread per
// location, float64.  mode 0 'Direct' (:262-264): (lon,lat)*pi/180, evaluated as (x*pi)/180 like
// the Python expression; mode 1 'Cartesian_3D' (:265-268, utils/utils.py:11-16): unit xyz of the
// radians above; mode 2 'Wrap' (positional_encoding/wrap.py:20-29): cos/sin of torch.deg2rad(x)
// = x * (pi/180) per column, ordered (cos lon, sin lon, cos lat, sin lat).
__global__ void coord_features_kernel(int mode, const double* __restrict__ lonlat, int64_t n,
                                      double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double lon = lonlat[2 * i], lat = lonlat[2 * i + 1];
    constexpr double PI = 3.141592653589793;
    if (mode == 2) {
        constexpr double PI_180 = 0.017453292519943295;
        const double a = lon * PI_180, b = lat * PI_180;
        out[4 * i + 0] = cos(a);
        out[4 * i + 1] = sin(a);
        out[4 * i + 2] = cos(b);
        out[4 * i + 3] = sin(b);
        return;
    }
    const double a = (lon * PI) / 180.0, b = (lat * PI) / 180.0;
    if (mode == 0) {
        out[2 * i + 0] = a;
        out[2 * i + 1] = b;
    } else {
        const double cb = cos(b);
        out[3 * i + 0] = cb * cos(a);
        out[3 * i + 1] = cb * sin(a);
        out[3 * i + 2] = sin(b);
    }
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

int range_blend(range_ctx* c, const float* G, const float* H, float beta, int64_t B, float* out,
                range_stream_t stream) {
    if (!c || !G || !H || !out) return fail(RANGE_ERR_INVALID, "null argument");
    if (B <= 0) return fail(RANGE_ERR_INVALID, "B must be > 0");
    ENTER_DEVICE(c);
    const int64_t n4 = B * (VAL_DIM / 4);
    return launch(blend_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, G, H, beta, n4, out);
}

// pass 1 with a running maximum (pass1_sharp.h); defined at the end of this file: hipcc emits kernels in the
// order of their first use, and the kernels of the default path keep theirs
static void (*sharp_scan_kernel(bool geo))(ScanArgs);
// the statistics from the kept logits (pass1_kept.h), likewise
static void (*kept_stats_kernel_for(int n_pairs, bool geo))(KeptStatsArgs);

// first_query / total_queries / force_splits: range_scan_stats_at (a scan in chunks whose
// kept logits share one workspace); a plain range_scan_stats is the chunk [0, B) of a scan of B.
static int scan_stats_impl(range_ctx* c, const float* ehat32, const float* xq32, int64_t B, float tau_sem,
                           float tau_geo, float* stats, int topk, float* topk_val, int64_t* topk_idx,
                           int32_t keep_logits, int64_t first_query, int64_t total_queries, int32_t force_splits,
                           range_stream_t stream) {
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
    HIP_TRY(c->pass.ws_stats_parts.ensure(p.part_floats));
    a.out = c->pass.ws_stats_parts.p;
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
    {
        ProfScope ps(c, RANGE_PROF_SCAN_STATS, s);
        void (*const kernel)(ScanArgs) = route.shift == SHIFT_RUNNING_MAX ? sharp_scan_kernel(geo) : scan_kernels[!geo][!topk_scan];
        if (int lrc = launch(kernel, dim3((unsigned)p.grid), dim3(256), SCAN_LDS_BYTES, s, a)) return lrc;
    }
    if (a.logits && keep_logits) {
        c->kept.kept_B = first_query + B;
        c->kept.kept_total = total_queries;
        c->kept.kept_blocks = a.n_blocks;
    }
    const int per_wg = p.merge_by_wave ? 4 : 256;      // queries of a merging workgroup: one per wave, or per thread
    rc = launch(p.merge_by_wave ? merge_stats_wave_kernel : merge_stats_kernel, dim3((unsigned)((B + per_wg - 1) / per_wg)),
                dim3(256), 0, s, c->pass.ws_stats_parts.p, a.n_splits, B, stats);
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
// chip, measured the same way as range_topk_stream_timed.  16-byte non-temporal loads, 8 in flight
// per thread, 1 024 workgroups; the xor of everything read goes to one word per workgroup so that
// the loads stay.
__global__ __launch_bounds__(256) void stream_read_kernel(const u32x4* __restrict__ p, int64_t n16, int passes,
                                                          uint32_t* __restrict__ sink) {
    // a workgroup reads 32 KB contiguous per step (8 loads of 16 bytes per thread, 4 KB apart)
    const int64_t step = (int64_t)gridDim.x * 2048;
    u32x4 acc = {0u, 0u, 0u, 0u};
    for (int ps = 0; ps < passes; ++ps) {
        for (int64_t base = (int64_t)blockIdx.x * 2048; base < n16; base += step) {
            u32x4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int64_t i = base + u * 256 + threadIdx.x;
                v[u] = __builtin_nontemporal_load(p + (i < n16 ? i : n16 - 1));
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) acc ^= v[u];
        }
    }
    uint32_t r = acc[0] ^ acc[1] ^ acc[2] ^ acc[3];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) r ^= __shfl_xor(r, off);
    if ((threadIdx.x & 63) == 0) atomicXor(sink + blockIdx.x, r);
}

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

int range_merge_stats(range_ctx* c, const float* parts, int32_t n_parts, int64_t B, float* out,
                      range_stream_t stream) {
    if (!c || !parts || !out) return fail(RANGE_ERR_INVALID, "null argument");
    if (n_parts <= 0 || B <= 0) return fail(RANGE_ERR_INVALID, "n_parts and B must be > 0");
    ENTER_DEVICE(c);
    const int tpb = 256;
    return launch(merge_stats_kernel, dim3((unsigned)((B + tpb - 1) / tpb)), dim3(tpb), 0,
                       (hipStream_t)stream, parts, n_parts, B, out);
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

// pass 2 into the context's split slabs; when `partial` is non-null the slabs are then summed
// (fixed order) into it, otherwise the caller consumes the slabs (n_splits_out of them) itself.
// kept_first >= 0: queries [kept_first, kept_first + B) of the last scan whose logits were kept
// (attend_stored_kernel; ehat32 is not read); kept_first < 0: recompute the logits.
// diag_dev non-null (range_attend_diag): the instrumented build of the recomputing kernel, always in
// the split scheme, with the slabs as its only output.
static int attend_impl(range_ctx* c, const float* ehat32, const float* xq32, int64_t B, float tau_sem,
                       float tau_geo, float beta, const float* stats_global, float* partial,
                       SlabMap* map_out, int64_t kept_first, range_stream_t stream,
                       unsigned long long* diag_dev = nullptr, int64_t diag_capacity = 0) {
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
    const Pass2Plan p = plan_pass2(c->n_cu, c->bank.n_rows, B, c->sw.p2_streamk && !bf16x3 && !diag_dev, PLAN_CONSTS);
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

int range_attend(range_ctx* c, const float* ehat32, const float* xq32, int64_t B, float tau_sem,
                 float tau_geo, float beta, const float* stats_global, float* partial,
                 range_stream_t stream) {
    if (!partial) return fail(RANGE_ERR_INVALID, "null argument");
    return attend_impl(c, ehat32, xq32, B, tau_sem, tau_geo, beta, stats_global, partial, nullptr, -1, stream);
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
    const int per_wg = p.merge_by_wave ? 4 : 256;      // queries of a merging workgroup: one per wave, or per thread
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
            if (int rc = launch(kept_stats_kernel_for(grp.count, a.geo_mask != 0u), dim3((unsigned)p.grid), dim3(256), 0, s, a)) return rc;
        }
        for (int i = 0; i < grp.count; ++i)
            if (int rc = launch(p.merge_by_wave ? merge_stats_wave_kernel : merge_stats_kernel, dim3((unsigned)((B + per_wg - 1) / per_wg)),
                                dim3(256), 0, s, c->kept.ws_stat_parts.p + (size_t)i * p.part_floats, p.n_splits, B,
                                stats + (size_t)(grp.first + i) * B * 4))
                return rc;
    }
    return RANGE_OK;
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

int range_finalize(range_ctx* c, const float* partials, int32_t n_parts, const double* ehat64,
                   int64_t B, double* out, range_stream_t stream) {
    if (!c || !partials || !ehat64 || !out) return fail(RANGE_ERR_INVALID, "null argument");
    if (n_parts <= 0 || B <= 0) return fail(RANGE_ERR_INVALID, "n_parts and B must be > 0");
    ENTER_DEVICE(c);
    const int64_t n = B * 320;
    return launch(finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, partials, SlabMap{n_parts, 0, 0, 0, 1}, ehat64, B, (int64_t)0, B, out);
}

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
    return RANGE_OK;
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

// encode -> pass 1 (keeping its logits) -> pass 2 into the context's split slabs; the caller
// finalizes (sums the slabs, packs with e-hat).  n_splits_out = number of slabs written.
static int forward_to_slabs(range_ctx* c, const double* lonlat, int64_t B, const ModelParams& m,
                            SlabMap* map_out, range_stream_t stream) {
    int rc = encode_to_workspace(c, lonlat, B, nullptr, stream);
    if (rc) return rc;
    rc = range_scan_stats(c, c->pass.ws_ehat32.p, c->pass.ws_xq.p, B, m.tau_sem, m.tau_geo, c->pass.ws_stats.p, 0,
                          nullptr, nullptr, /*keep_logits=*/1, stream);
    if (rc) return rc;
    // pass 2 consumes the logits pass 1 kept (recomputes them if they did not fit in memory)
    return attend_impl(c, c->pass.ws_ehat32.p, c->pass.ws_xq.p, B, m.tau_sem, m.tau_geo, m.beta, c->pass.ws_stats.p,
                       nullptr, map_out, c->kept.kept_B == B ? 0 : -1, stream);
}

int range_forward(range_ctx* c, const double* lonlat, int64_t B, int32_t model, float beta,
                  double* out, range_stream_t stream) {
    if (!c || !lonlat || !out) return fail(RANGE_ERR_INVALID, "null argument");
    ModelParams m;
    if (int rc = model_params(c, model, beta, m)) return rc;
    c->pass.ws_queries = 0;
    if (plan_temperatures(m.tau_sem, m.tau_geo, B, c->sw.small_forward).one_pass) {
        // a handful of queries: one pass over the bank (attend_small.h)
        if (int lrc = encode_to_workspace(c, lonlat, B, nullptr, stream)) return lrc;
        c->pass.ws_queries = B;
        ENTER_DEVICE(c);
        return forward_small(c, B, m, out, (hipStream_t)stream);
    }
    // single GPU: the finalize kernel sums the split slabs itself (same fixed order as
    // reduce_parts_kernel, so the result is bit-identical to attend + finalize)
    SlabMap map{};
    if (int lrc = forward_to_slabs(c, lonlat, B, m, &map, stream)) return lrc;
    c->pass.ws_queries = B;
    ENTER_DEVICE(c);
    const int64_t n = B * 320;
    return launch(finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                  c->pass.ws_slabs.p, map, c->pass.ws_ehat64.p, B, (int64_t)0, B, out);
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
    if (!c || !lonlat || !out_host) return fail(RANGE_ERR_INVALID, "null argument");
    ModelParams m;
    if (int rc0 = model_params(c, model, beta, m)) return rc0;
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
    rc = range_scan_stats(c, c->pass.ws_ehat32.p, c->pass.ws_xq.p, B, m.tau_sem, m.tau_geo, c->pass.ws_stats.p, 0,
                          nullptr, nullptr, /*keep_logits=*/1, stream);
    if (rc) return rc;
    const bool kept = c->kept.kept_B == B;

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
        rc = attend_impl(c, c->pass.ws_ehat32.p + p0 * 256, c->pass.ws_xq.p + p0 * 4, p1 - p0, m.tau_sem, m.tau_geo, m.beta,
                         c->pass.ws_stats.p + p0 * 4, nullptr, &map, kept ? p0 : -1, stream);
        if (rc) { (void)hipDeviceSynchronize(); give_back(); return rc; }
        // finalize per slab (the split slabs of this part are overwritten by the next part's pass 2,
        // which is behind these kernels in stream order)
        // (the last part in slabs of 256 queries: its copies and fills are what the caller waits for,
        // and they pipeline per slab)
        const int64_t slab = part + 2 == cuts.size() && cuts.size() > 2 ? SLAB / 4 : SLAB;
        for (int64_t q0 = p0; q0 < p1 && e == hipSuccess; q0 += slab) {
            Slab sl{q0, std::min<int64_t>(slab, p1 - q0), c->get_event(), c->get_event()};
            slabs.push_back(sl);
            const int64_t n = sl.nq * 320;
            hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                               c->pass.ws_slabs.p, map, c->pass.ws_ehat64.p + p0 * 256, p1 - p0, q0 - p0, sl.nq,
                               c->host.ws_out64.p + p0 * RANGE_OUT_DIM);
            e = hipGetLastError();
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

int range_profile_enable(range_ctx* c, int32_t on) {
    if (!c) return fail(RANGE_ERR_INVALID, "null argument");
    ENTER_DEVICE(c);
    for (auto& v : c->prof.pairs) {
        for (auto& p : v) { (void)hipEventSynchronize(p.second); c->ev_pool.push_back(p.first); c->ev_pool.push_back(p.second); }
        v.clear();
    }
    c->prof.on = on != 0;
    return RANGE_OK;
}

int range_profile_read(range_ctx* c, int32_t which, double* total_ms, int32_t* launches) {
    if (!c || which < 0 || which >= RANGE_PROF_KINDS || !total_ms || !launches) return fail(RANGE_ERR_INVALID, "bad argument");
    ENTER_DEVICE(c);
    double sum = 0.0;
    for (auto& p : c->prof.pairs[which]) {
        HIP_TRY(hipEventSynchronize(p.second));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, p.first, p.second));
        sum += ms;
    }
    *total_ms = sum;
    *launches = (int32_t)c->prof.pairs[which].size();
    return check_async_error(c);     // (the events above synchronised: a give-up of the profiled calls is known now)
}

int range_last_attend_geometry(const range_ctx* c, int32_t* n_query_tiles, int32_t* n_splits) {
    if (!c) return fail(RANGE_ERR_INVALID, "null argument");
    if (n_query_tiles) *n_query_tiles = c->pass.last_qtiles;
    if (n_splits) *n_splits = c->pass.last_splits;
    return RANGE_OK;
}

}  // extern "C"

#include "posenc_host.h"   // (the side encoders' host code, each with its kernel tables: in this order, around the two below)

static void (*sharp_scan_kernel(bool geo))(ScanArgs) {
    // [0: with the geographic head, 1: without]
    static void (*const sharp_kernels[2])(ScanArgs) = {sharp_scan_stats_kernel<true>, sharp_scan_stats_kernel<false>};
    return sharp_kernels[!geo];
}

static void (*kept_stats_kernel_for(int n_pairs, bool geo))(KeptStatsArgs) {
    // [pairs of the launch - 1][0: some pair has a geographic head, 1: none]
    static void (*const kept_kernels[KEPT_MAX_PAIRS][2])(KeptStatsArgs) = {
        {kept_stats_kernel<1, true>, kept_stats_kernel<1, false>}, {kept_stats_kernel<2, true>, kept_stats_kernel<2, false>},
        {kept_stats_kernel<3, true>, kept_stats_kernel<3, false>}, {kept_stats_kernel<4, true>, kept_stats_kernel<4, false>},
        {kept_stats_kernel<5, true>, kept_stats_kernel<5, false>}, {kept_stats_kernel<6, true>, kept_stats_kernel<6, false>},
        {kept_stats_kernel<7, true>, kept_stats_kernel<7, false>}, {kept_stats_kernel<8, true>, kept_stats_kernel<8, false>}};
    return kept_kernels[n_pairs - 1][!geo];
}

#include "csp_host.h"
#include "checker_host.h"
#include "neighbor_host.h"
