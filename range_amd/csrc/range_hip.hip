// librange_hip.so - C ABI (include/range_hip.h) over the hand-written gfx950 kernels.
// Host side of the engine, one translation unit: the kernel headers, the context (engine_ctx.h) and the entry
// points by stage (*_host.h); this file keeps create / destroy, the async-error words, the temperatures, profiling.
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
#include "../../include/range_headfit.h"
#include "../../include/range_cspfit.h"
#include "host_common.h"
#include "host_copy.h"
#include "host_plan.h"
#include "scan_common.h"
#include "topk_lists.h"
#include "pass1.h"
#include "pass1_sharp.h"
#include "pass1_kept.h"
#include "pass2.h"
#include "pass1_beside.h"
#include "topk_stream.h"
#include "topk_gemm.h"
#include "attend_bf16x3.h"
#include "attend_small.h"
#include "encoder_kernel.h"
#include "posenc_kernel.h"
#include "csp_kernel.h"
#include "csp_head_kernel.h"
#include "csp_rank_kernel.h"
#include "headfit_kernels.h"
#include "cspfit_kernels.h"
#include "checker_kernel.h"
#include "neighbor_kernel.h"
#include "kde_kernel.h"

using namespace range_hip;
using namespace range_host;

#include "engine_ctx.h"
// the retrieval engine's entry points, by stage (each uses what the ones above it define) ...
#include "encoder_host.h"
#include "bank_host.h"
#include "scan_host.h"
#include "topk_host.h"
#include "forward_host.h"
// ... and the side encoders'
#include "posenc_host.h"
#include "csp_host.h"
#include "headfit_host.h"
#include "cspfit_host.h"
#include "checker_host.h"
#include "neighbor_host.h"
#include "kde_host.h"

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

// (check_async_error itself is in engine_ctx.h: the encoder, top-k and forward calls run it)
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

// the give-up words as data, in stream order (async_err.h: async_flag_kernel)
int range_async_error_flag(range_ctx* c, double* flag_dev, range_stream_t stream) {
    if (!c || !flag_dev) return fail(RANGE_ERR_INVALID, "null argument");
    ENTER_DEVICE(c);
    if (!c->d_async_err) {            // (no host-mapped words in this context: nothing can have been reported)
        HIP_TRY(hipMemsetAsync(flag_dev, 0, sizeof(double), (hipStream_t)stream));
        return RANGE_OK;
    }
    return launch(async_flag_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, c->d_async_err, flag_dev);
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

}  // extern "C"
