// The evaluation the CSP class head exists for (location_models/csp/main/eval_helper.py: compute_acc_batch /
// get_label_rank): per row b with label t, over the scores s_c = (double) p_c * (double) img[b, c] of all classes -
// p_c the head's float32 probability, the bits range_csp_head(PROBS) gives; without image predictions s_c =
// (double) p_c, without embeddings ('no_prior') s_c = (double) img[b, c] -
//   greater[b]    : classes c != t with s_c > s_t or s_c NaN
//   tied_after[b] : classes c > t with s_c == s_t          (rank = 1 + greater + tied_after)
//   argmax[b]     : the first index of the maximum, the first NaN if there is one (np.argmax)
// all three -1 where s_t is NaN, -2 where the label is outside [0, C).  The (B, C) matrix is never written.
// host_plan.h: csp_rank_plan.
//
// ARITHMETIC.  The head's: csp_head_kernel.h's X tile, column gather and k-ordered float32 MFMA chain, its
// csp_activation<SIGMOID>.  A row tile first runs the head's subset path with the tile's labels as the id array -
// T columns for T rows, wave m the column tile of rows 32 m .. - and keeps the diagonal, s_t, in LDS: the chain
// of the sweep's column t, so that s_c > s_t is never decided by two roundings.  Then the item's chunks are swept
// as the head sweeps them; where the head stores a probability, this kernel loads the image prediction of the
// same row and column (per accumulator register 32 lanes read 32 consecutive columns of one row), multiplies in
// float64 and compares.
//
// STATE.  No running state in registers (the head's budget - two workgroups a CU - is kept): per wave and row,
// in LDS, {s_t, best score} (one 16-byte read per element), the best index and the two counts.  A compare's
// ballot gives the 32 lanes' count of a row as a population count; lane 0 of the row adds it.  The best pair
// changes about ln C times a row: the wave takes the slow path (a fixed xor tree over the row's 32 lanes: larger
// score, NaN first, lower column on equality) only when some lane beats the row's best.  At the end of the item
// one thread a row folds the four waves in wave order - integers and (score, index) pairs by the same rule: the
// result does not depend on B, the grid or the stream.
//
// PARTS.  With col_parts > 1 item = row tile * col_parts + part sweeps its share of the chunks and writes partial
// (greater, tied_after, best score, best index) to the workspace; csp_rank_merge_kernel folds the parts in order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csp_head_kernel.h"
#include "host_plan.h"

namespace range_hip {

using range_host::CSP_IMG_F32;
using range_host::CSP_IMG_F64;
using range_host::CSP_IMG_NONE;

constexpr int32_t CSP_RANK_NO_INDEX = 0x7fffffff;   // no column beat -inf yet: the row is all -inf so far
constexpr int32_t CSP_RANK_NAN = -1, CSP_RANK_BAD_LABEL = -2;

struct CspRankArgs {
    const float* x;          // (B, K) float32, or null (HEAD = false)
    const float4* w4;        // packed class_emb
    const void* img;         // (B, C) float32 / float64, or null (IMG = CSP_IMG_NONE)
    const int32_t* labels;   // (B)
    int32_t *greater, *tied, *argmax;       // (B) each
    // col_parts > 1: (col_parts, B) partial results
    double* ws_best;
    int32_t *ws_greater, *ws_tied, *ws_index;
    int64_t B, n_items;
    int32_t K, k_groups, ld, C, col_tiles, n_chunks, col_parts;
};

struct CspRankRow {          // per wave and row
    double st, best;
};

template <int IMG>
__device__ __forceinline__ double csp_rank_img(const void* img, int64_t at) {
    if (IMG == CSP_IMG_F32) return (double)static_cast<const float*>(img)[at];
    if (IMG == CSP_IMG_F64) return static_cast<const double*>(img)[at];
    return 1.0;
}

// (sa, ia) comes before (sb, ib) in np.argmax's order: NaN first, then the larger score, the lower index on equality
__device__ __forceinline__ bool csp_rank_before(double sa, int32_t ia, double sb, int32_t ib) {
    const bool na = sa != sa, nb = sb != sb;
    if (na || nb) return na && (!nb || ia < ib);
    return sa > sb || (sa == sb && ia < ib);
}

// Some lane of a row's 32 holds a pair (s, i) that beats the row's best; the others (-inf, CSP_RANK_NO_INDEX).  The
// best of them by a fixed xor tree inside the half wave; lane 0 of the row writes it.
__device__ __forceinline__ void csp_rank_new_best(double s, int32_t i, CspRankRow* row, int32_t* index, int l31) {
    double bs = i != CSP_RANK_NO_INDEX ? s : -__builtin_inf();
    int32_t bi = i;
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) {
        const double os = __shfl_xor(bs, o);
        const int32_t oi = __shfl_xor(bi, o);
        if (csp_rank_before(os, oi, bs, bi)) { bs = os; bi = oi; }
    }
    if (l31 == 0 && bi != CSP_RANK_NO_INDEX) {
        row->best = bs;
        *index = bi;
    }
    // the wave's later reads of the row come behind the write (LDS serves a wave in order)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// (two waves a SIMD, not more: the X tile's LDS allows two workgroups a CU at most, and an allocator that aims at
// three spills the sweep's accumulators)
template <int MT, int IMG, bool HEAD>
__global__ __launch_bounds__(CSP_BLOCK, 2) __attribute__((amdgpu_waves_per_eu(2, 2))) void csp_rank_kernel(CspRankArgs a) {
    constexpr int T = 32 * MT;
    constexpr int NT = CSP_HEAD_ACC_TILES / MT;
    extern __shared__ __attribute__((aligned(16))) float csp_hx[];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l31 = lane & 31, lh = lane >> 5;
    const int ld = a.ld, K = a.K, k_pad = a.k_groups * 8;
    // behind the X tile (HEAD; 16-byte aligned: T ld floats, T a multiple of 32): (4, T) rows, (T) s_t, (4, T) best
    // indices, (4, T) greater, (4, T) tied, (T) labels
    CspRankRow* const rows = reinterpret_cast<CspRankRow*>(csp_hx + (HEAD ? T * ld : 0));
    double* const st = reinterpret_cast<double*>(rows + 4 * T);
    int32_t* const bidx = reinterpret_cast<int32_t*>(st + T);
    int32_t* const cgt = bidx + 4 * T;
    int32_t* const ctie = cgt + 4 * T;
    int32_t* const lab = ctie + 4 * T;
    const bool vec4 = K % 4 == 0 && reinterpret_cast<uintptr_t>(a.x) % 16 == 0;
    const double ninf = -__builtin_inf();
    int64_t loaded = -1;
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const int64_t rt = item / a.col_parts;
        const int part = (int)(item - rt * a.col_parts);
        const int ch0 = (int)((int64_t)part * a.n_chunks / a.col_parts);
        const int ch1 = (int)((int64_t)(part + 1) * a.n_chunks / a.col_parts);
        const int64_t b0 = rt * T;
        const int live_rows = a.B - b0 < T ? (int)(a.B - b0) : T;
        __syncthreads();                        // the last item's reads of the tile and of the state are done
        if (HEAD && rt != loaded) {
            csp_head_load_x<T>(a.x, a.B, b0, K, k_pad, ld, vec4, csp_hx, wave, lane);
            loaded = rt;
        }
        if (t < T) lab[t] = t < live_rows ? a.labels[b0 + t] : 0;
        __syncthreads();
        // s_t of the tile's rows
        if (HEAD) {
            if (wave < MT) {
                // the head's subset path: column c of this "call" is the class labels[b0 + c]
                uint32_t base[NT];
                int col[NT];
                csp_head_columns<NT>(base, col, wave, l31, lh, a.labels + b0, live_rows, a.C, a.k_groups);
                csp_f32x16 acc[MT][NT];
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int j = 0; j < NT; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[m][j][r] = 0.0f;
                csp_head_gemm_dispatch<MT, NT>(acc, 1, a.w4, base, a.k_groups, csp_hx + l31 * ld + lh, 32 * ld);
                // the diagonal of tile (m = wave, j = 0): element r of a lane is row (r & 3) + 8 (r >> 2) + 4 lh, column
                // l31 - the lanes with lh = bit 2 of l31 hold it at r = (l31 & 3) + 4 (l31 >> 3)
                float z = 0.0f;
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (m == wave && r == (l31 & 3) + 4 * (l31 >> 3)) z = acc[m][0][r];
                const int row = 32 * wave + l31;
                if (lh == ((l31 >> 2) & 1)) {
                    const int id = lab[row];
                    double s = 0.0;
                    if (row < live_rows && id >= 0 && id < a.C)
                        s = (double)csp_activation<range_host::CSP_ACT_SIGMOID>(z) * csp_rank_img<IMG>(a.img, (b0 + row) * a.C + id);
                    st[row] = s;
                }
            }
        } else if (t < T) {
            const int id = lab[t];
            st[t] = t < live_rows && id >= 0 && id < a.C ? csp_rank_img<IMG>(a.img, (b0 + t) * a.C + id) : 0.0;
        }
        __syncthreads();
        if (lane < T) {
            rows[wave * T + lane] = CspRankRow{st[lane], ninf};
            bidx[wave * T + lane] = CSP_RANK_NO_INDEX;
            cgt[wave * T + lane] = 0;
            ctie[wave * T + lane] = 0;
        }
        __syncthreads();
        CspRankRow* const wrows = rows + wave * T;
        int32_t* const wbidx = bidx + wave * T;
        int32_t* const wgt = cgt + wave * T;
        int32_t* const wtie = ctie + wave * T;
        for (int ch = ch0; ch < ch1; ++ch) {
            const int t0 = ch * 4 * NT + wave;
            int ntw = a.col_tiles > t0 ? (a.col_tiles - t0 + 3) / 4 : 0;
            ntw = ntw < NT ? ntw : NT;
            if (ntw == 0) continue;
            uint32_t base[NT];
            int col[NT];
            csp_head_columns<NT>(base, col, t0, l31, lh, nullptr, a.C, a.C, a.k_groups);
            csp_f32x16 acc[MT][NT];
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[m][j][r] = 0.0f;
            // The image predictions of the tile, in the accumulators' layout: element r of tile (m, j) is row (r & 3) +
            // 8 (r >> 2) + 4 lh of the row tile's 32 m .., column col[j] (a row beyond B reads the tile's last row; its
            // results are not written).  A row block m at a time behind the MFMAs, as ONE batch of loads in flight
            // (32 or 64 registers - requesting the whole tile before the MFMAs spills the accumulators' neighbours).
            // (addressed as the tile's uniform base plus a 32-bit element offset - at most 64 x 32768 - formed at the
            // load: 64 full addresses would take the registers the values need)
            const auto img_at = [&](int m, int j, int r) {
                const int row = m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                return (uint32_t)((row < live_rows ? row : live_rows - 1) * a.C + (col[j] < a.C ? col[j] : a.C - 1));
            };
            const int64_t tile_at = b0 * a.C;
            if (HEAD) csp_head_gemm_dispatch<MT, NT>(acc, ntw, a.w4, base, a.k_groups, csp_hx + l31 * ld + lh, 32 * ld);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                float gf[IMG == CSP_IMG_F32 ? NT : 1][16];
                double gd[IMG == CSP_IMG_F64 ? NT : 1][16];
                if (IMG == CSP_IMG_F32) {
#pragma unroll
                    for (int j = 0; j < NT; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            gf[j][r] = j < ntw ? (static_cast<const float*>(a.img) + tile_at)[img_at(m, j, r)] : 0.0f;
                }
                if (IMG == CSP_IMG_F64) {
#pragma unroll
                    for (int j = 0; j < NT; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            gd[j][r] = j < ntw ? (static_cast<const double*>(a.img) + tile_at)[img_at(m, j, r)] : 0.0;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    int ngt = 0, ntie = 0;          // of this row's 32 lanes, over the wave's tiles of the chunk
                    const CspRankRow rr = wrows[row];
                    // the lane's best of its columns of this row that beat the row's best so far (columns ascend with
                    // j: the first occurrence stays; behind a NaN nothing beats)
                    double cur = rr.best;
                    int32_t ci = CSP_RANK_NO_INDEX;
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        if (j < ntw) {              // (wave-uniform)
                            const bool valid = col[j] < a.C;
                            double s = HEAD ? (double)csp_activation<range_host::CSP_ACT_SIGMOID>(acc[m][j][r]) : 1.0;
                            if (IMG != CSP_IMG_NONE) {
                                const double g = IMG == CSP_IMG_F32 ? (double)gf[IMG == CSP_IMG_F32 ? j : 0][r]
                                                                    : gd[IMG == CSP_IMG_F64 ? j : 0][r];
                                s = HEAD ? s * g : g;
                            }
                            // (column t itself is s_t's own chain: never greater, unless NaN - then the row is flagged)
                            const uint64_t mgt = __ballot(valid && !(s <= rr.st)), meq = __ballot(valid && s == rr.st);
                            ngt += lh ? __popc((uint32_t)(mgt >> 32)) : __popc((uint32_t)mgt);
                            if (meq) {
                                const uint64_t mtie = __ballot(valid && s == rr.st && col[j] > lab[row]);
                                ntie += lh ? __popc((uint32_t)(mtie >> 32)) : __popc((uint32_t)mtie);
                            }
                            if (valid && cur == cur && !(s <= cur)) { cur = s; ci = col[j]; }
                        }
                    }
                    if (__builtin_expect(__ballot(ci != CSP_RANK_NO_INDEX) != 0, 0))
                        csp_rank_new_best(cur, ci, wrows + row, wbidx + row, l31);
                    if (l31 == 0) {
                        wgt[row] += ngt;
                        wtie[row] += ntie;
                    }
                }
            }
        }
        __syncthreads();
        if (t < live_rows) {
            const int32_t label = lab[t];
            const double s_t = st[t];
            int32_t g = 0, e = 0, bi = CSP_RANK_NO_INDEX;
            double bs = ninf;
            for (int w = 0; w < 4; ++w) {
                g += cgt[w * T + t];
                e += ctie[w * T + t];
                const double os = rows[w * T + t].best;
                const int32_t oi = bidx[w * T + t];
                if (oi != CSP_RANK_NO_INDEX && csp_rank_before(os, oi, bs, bi)) { bs = os; bi = oi; }
            }
            const int32_t flag = label < 0 || label >= a.C ? CSP_RANK_BAD_LABEL : s_t != s_t ? CSP_RANK_NAN : 0;
            if (a.col_parts > 1) {
                const int64_t at = (int64_t)part * a.B + b0 + t;
                a.ws_greater[at] = flag ? flag : g;
                a.ws_tied[at] = e;
                a.ws_best[at] = bs;
                a.ws_index[at] = bi;
            } else {
                a.greater[b0 + t] = flag ? flag : g;
                a.tied[b0 + t] = flag ? flag : e;
                a.argmax[b0 + t] = flag ? flag : bi == CSP_RANK_NO_INDEX ? 0 : bi;
            }
        }
    }
}

// the parts of a row in part order: counts added, the best pair by np.argmax's order
__global__ __launch_bounds__(CSP_BLOCK) void csp_rank_merge_kernel(CspRankArgs a) {
    for (int64_t b = (int64_t)blockIdx.x * CSP_BLOCK + threadIdx.x; b < a.B; b += (int64_t)gridDim.x * CSP_BLOCK) {
        int32_t g = 0, e = 0, bi = CSP_RANK_NO_INDEX;
        double bs = -__builtin_inf();
        const int32_t flag = a.ws_greater[b] < 0 ? a.ws_greater[b] : 0;     // every part flags a row alike
        for (int p = 0; p < a.col_parts; ++p) {
            const int64_t at = (int64_t)p * a.B + b;
            g += a.ws_greater[at];
            e += a.ws_tied[at];
            const double os = a.ws_best[at];
            const int32_t oi = a.ws_index[at];
            if (oi != CSP_RANK_NO_INDEX && csp_rank_before(os, oi, bs, bi)) { bs = os; bi = oi; }
        }
        a.greater[b] = flag ? flag : g;
        a.tied[b] = flag ? flag : e;
        a.argmax[b] = flag ? flag : bi == CSP_RANK_NO_INDEX ? 0 : bi;
    }
}

}  // namespace range_hip
