// Words of a context's host-mapped error area (engine_ctx.h: range_ctx::h_async_err), set to 1 - a
// plain system-scope store - by a persistent kernel whose bounded in-launch wait for other
// workgroups gave up.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace range_hip {
constexpr int RANGE_ASYNC_WORD_ENCODER = 0;   // encoder_tile_kernel: the tile's rows were written as NaN
constexpr int RANGE_ASYNC_WORD_TOPK = 1;      // topks_tail: the query's results were written as NaN / -1
}  // namespace range_hip

// The give-up words as DATA, in stream order (range_hip.h: range_async_error_flag): a rank of a
// row-sharded job sends this with its rows, so that every rank learns from the WORD - not from NaN in
// the data, which a NaN coordinate produces as well - that a peer's persistent launch gave up.
// (extern "C": the symbol is the plain name)
extern "C" __global__ void async_flag_kernel(const uint32_t* __restrict__ err, double* __restrict__ flag) {
    using namespace range_hip;
    if (threadIdx.x == 0 && blockIdx.x == 0)
        flag[0] = (__hip_atomic_load(err + RANGE_ASYNC_WORD_ENCODER, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) |
                   __hip_atomic_load(err + RANGE_ASYNC_WORD_TOPK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) ? 1.0 : 0.0;
}
