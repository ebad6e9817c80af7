// The merge of the stream top-k's candidate lists (one query per workgroup), the float32 similarity
// chain it re-ranks with, and the brute-force path behind its exactness check.
//
// A part of topk_stream.h, which includes it between the lists' publication and the tail that
// calls the merge (TopkStreamArgs, TOPKS_*, ld_agent come from there): include topk_stream.h.
#pragma once

namespace range_hip {

// The merge of one query: 256 threads, thread p owns the sorted list (L keys) of stream
// workgroup p (n_parts <= 256).  Runs as the tail of the stream kernels (topks_tail) or as
// topk_merge_kernel (one workgroup per query) when the batch has more queries than workgroups.
//  1. a lower bound T of the query's 16th best value: the 16th largest list head (rank by
//     counting over the 256 heads in LDS) - each head is the maximum of a different row set, so
//     sixteen candidates are >= T.  Entries below T cannot be in the top 16.
//  2. the survivors (>= T; a few dozen of the 2048 entries) are compacted into LDS and ranked by
//     counting; ranks 0..k-1 are the result, already in order (keys are unique).
//  3. exactness of the short lists: if the largest value any lane, wave or workgroup let go
//     reaches the k-th value found (or `force_exact`), the query is recomputed by brute force
//     over all rows, each thread walking its rows with the SAME fmaf chain as the MFMA (k order:
//     for s, for component, for lane group) and full 16-deep lists.  exact_count (optional)
//     counts the queries that took that path.
//  Prefilter form (eps_rel > 0: the candidates carry APPROXIMATE values from bf16 keys, within
//  eps = eps_rel |q| kmax of the float32 similarity): the threshold of step 1 is lowered by 2 eps,
//  step 2 ranks the survivors by approximate value to find the k-th best approximate value v_k,
//  step 3 widens the check to dall >= v_k - 2 eps, and then every survivor >= v_k - 2 eps gets its
//  float32 similarity by the fmaf chain of the brute-force path (16 lanes per survivor, 1 KB of
//  key row each) and the survivors are ranked again by those: the result is that of the float32 scan.
constexpr int TOPKM_CAP = 256 * TOPKS_WL;    // every entry of every list
constexpr int TOPKM_OFF_SURV2 = TOPKM_CAP * 8;
constexpr int TOPKM_OFF_SH = 2 * TOPKM_CAP * 8;              // brute force: 16 x MAX_TOPK keys
constexpr int TOPKM_OFF_RES = TOPKM_OFF_SH + 16 * MAX_TOPK * 8;
constexpr int TOPKM_OFF_HEAD = TOPKM_OFF_RES + MAX_TOPK * 8;
constexpr int TOPKM_OFF_Q = TOPKM_OFF_HEAD + 256 * 4;
constexpr int TOPKM_OFF_F = TOPKM_OFF_Q + KEY_DIM * 4;
constexpr int TOPKM_OFF_I = TOPKM_OFF_F + 8 * 4;
constexpr int TOPKM_OFF_X = TOPKM_OFF_I + 16;                // transpose area of topk_exact_values: 64 padded key rows
constexpr int TOPKM_LDS_BYTES = TOPKM_OFF_X + 64 * 4 * (256 + 16);

// the similarity every float32 kernel computes: acc = fmaf(K[16 s + 4 g + c], Q[16 s + 4 g + c], acc)
// in the order s = 0..15, c = 0..3, g = 0..3 of the MFMA chain.  The key row is loaded S steps (of 16
// dimensions) at a time: S = 1 where the threads of a workgroup walk a whole bank (sixteen dependent
// groups of four loads; the loop over them is left to hipcc), S = 8 where a thread evaluates one row
// of its own and would pay the memory latency sixteen times (two bursts of 32 loads instead).
template <int S>
__device__ __forceinline__ float topk_exact_dot(const float* __restrict__ kr, const float* sh_q) {
    static_assert(S == 1 || S == 8, "the rolled walk and the two-burst form");
    float acc = 0.f;
    for (int s0 = 0; s0 < 16; s0 += S) {
        f32x4 kc[4 * S];
#pragma unroll
        for (int i = 0; i < 4 * S; ++i) kc[i] = *reinterpret_cast<const f32x4*>(kr + 16 * s0 + 4 * i);
#pragma unroll
        for (int s = 0; s < S; ++s) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
#pragma unroll
                for (int gg = 0; gg < 4; ++gg)
                    acc = __builtin_fmaf(kc[4 * s + gg][c], sh_q[16 * (s0 + s) + 4 * gg + c], acc);
            }
        }
    }
    return acc;
}
__device__ __forceinline__ uint32_t topk_ordered_bits(float v) { return (uint32_t)(topk_key(v, 0u) >> 32); }

// The brute-force path of the merge: every row's float32 similarity, full 16-deep lists, wave
// merges through `sh` (16 x MAX_TOPK keys), result in res[0..MAX_TOPK).  Inlined: a call would
// give the stream kernels a stack (scratch memory set up at every dispatch).
__device__ __forceinline__ void topk_brute_force(const float* __restrict__ keys, int64_t n_valid,
                                                           const float* sh_q, unsigned long long* sh,
                                                           unsigned long long* res) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_wv = blockDim.x >> 6;
    KeyList X;
    X.init();
    for (int64_t row = threadIdx.x; row < n_valid; row += blockDim.x)
        X.push(topk_key(topk_exact_dot<1>(keys + row * KEY_DIM, sh_q), (uint32_t)row));
    merge_wave(X);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < MAX_TOPK; ++i) sh[wave * MAX_TOPK + i] = X.k[i];
    }
    __syncthreads();
    if (wave == 0) {
        KeyList M;
        M.init();
        if (lane < n_wv) {
#pragma unroll
            for (int i = 0; i < MAX_TOPK; ++i) M.k[i] = sh[lane * MAX_TOPK + i];
        }
        merge_wave(M);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < MAX_TOPK; ++i) res[i] = M.k[i];
        }
    }
    __syncthreads();
}

// value of lane l-1 of this lane's row of 16 (lane 0 of a row: 0.0f) - one DPP move
__device__ __forceinline__ float topk_row_shr1(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, false));
}

// largest value of the wave, in every lane: two quad permutes and two mirrors inside each row of 16
// (DPP operands of v_max_u32), then the four row results through scalar registers
__device__ __forceinline__ uint32_t topk_wave_umax(uint32_t v) {
    uint32_t t;
    t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false); v = t > v ? t : v;    // quad_perm [1,0,3,2]
    t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false); v = t > v ? t : v;    // quad_perm [2,3,0,1]
    t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false); v = t > v ? t : v;   // row_half_mirror
    t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, false); v = t > v ? t : v;   // row_mirror
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 16),
                   r2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), r3 = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
    const uint32_t a = r0 > r1 ? r0 : r1, b = r2 > r3 ? r2 : r3;
    return a > b ? a : b;
}

struct TopkMergeLds {
    unsigned long long *surv, *surv2, *sh, *res;
    uint32_t* sh_head;
    float *sh_q, *sh_d, *sh_n2;
    int* sh_i;
    __device__ __forceinline__ explicit TopkMergeLds(char* lds)
        : surv(reinterpret_cast<unsigned long long*>(lds)),
          surv2(reinterpret_cast<unsigned long long*>(lds + TOPKM_OFF_SURV2)),
          sh(reinterpret_cast<unsigned long long*>(lds + TOPKM_OFF_SH)),
          res(reinterpret_cast<unsigned long long*>(lds + TOPKM_OFF_RES)),
          sh_head(reinterpret_cast<uint32_t*>(lds + TOPKM_OFF_HEAD)),
          sh_q(reinterpret_cast<float*>(lds + TOPKM_OFF_Q)),
          sh_d(reinterpret_cast<float*>(lds + TOPKM_OFF_F)),          // [4] dmax per wave (ordered bits)
          sh_n2(reinterpret_cast<float*>(lds + TOPKM_OFF_F) + 4),     // [4] the waves' shares of |q| (norms, not squares)
          sh_i(reinterpret_cast<int*>(lds + TOPKM_OFF_I)) {}          // survivor count, flag
};

// what the merge of query q needs and nobody else writes: the query itself (float32 similarities
// of the survivors / brute force) and its norm.  In the fused tail this runs BEFORE the wait for
// the other workgroups.  256 threads.
template <int L>
__device__ void topk_merge_prefetch(char* lds, int64_t q, const TopkStreamArgs& a) {
    TopkMergeLds m(lds);
    const int p = threadIdx.x;                                        // blockDim.x == 256 == KEY_DIM
    const float v = a.ehat[q * KEY_DIM + p];
    m.sh_q[p] = v;
    // the wave's share of |q|, taken of the elements times the power of two that brings the wave's largest
    // near 1 (a query of norm 1e-25 squared in float32 is 0 - and a zero error bound made the merge hand out
    // the APPROXIMATE values as if they were exact; found by tests/test_gpu_topk_gemm.py in round 5)
    float mx = fabsf(v);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    const uint32_t mE = (__float_as_uint(mx) >> 23) & 0xFFu;
    const float up = (mE >= 1u && mE <= 253u) ? __uint_as_float((254u - mE) << 23) : 1.0f;     // 2^(127 - E)
    const float vs = v * up;
    float sq = vs * vs;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) sq += __shfl_xor(sq, off);
    if ((p & 63) == 0) m.sh_n2[p >> 6] = sqrtf(sq) / up;              // (a NORM per wave, not a square)
    if (p == 0) { m.sh_i[0] = 0; m.sh_i[1] = 0; }
    if (p < MAX_TOPK) m.res[p] = 0ull;
}

// ranks (by counting) of the S keys of `src`; ranks 0..15 land in res[] in order (keys are unique)
__device__ __forceinline__ void topk_rank_into(const unsigned long long* src, int S, unsigned long long* res) {
    for (int t = threadIdx.x; t < S; t += 256) {
        const unsigned long long key = src[t];
        if (key == 0ull) continue;
        int r = 0;
        for (int u = 0; u < S; ++u) r += src[u] > key ? 1 : 0;
        if (r < MAX_TOPK) res[r] = key;
    }
}

// float32 similarities of the survivors whose (approximate) value is >= vmin: surv2[t] = key of
// (exact value, row), 0 for the others.  4 lanes per survivor (64 at a time).
//  * loads: 16 instructions, the quad of a survivor reading 64 contiguous bytes of its key row in
//    each (with one lane reading a contiguous quarter row the 64 lanes of an instruction hit 64
//    different cache lines: measured 2.7 us for this step, most of it the tag lookups);
//  * through LDS (rows of 4 quarters, each padded by 16 B so that both the writes above and the
//    reads below are bank-conflict free) every lane s then holds dims 64 s .. 64 s + 63;
//  * the chain runs chunk by chunk in the kernels' order, its value handed from a lane to the
//    next by a DPP row shift (every lane computes on its own four chunks at every step; at step
//    s only lane s has the right input, and lane 3 ends with the result).  The 256 fmaf of a
//    similarity are one dependent chain whatever the split.
constexpr int TOPKM_XROW = 4 * (256 + 16);                   // a key row in the transpose area
__device__ __forceinline__ void topk_exact_values(const TopkStreamArgs& a, const float* sh_q, char* xarea,
                                                  const unsigned long long* surv, unsigned long long* surv2, int S, float vmin) {
    const int p = threadIdx.x, sub = p & 3, cand = p >> 2;
    f32x4 qc[4][4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) qc[h][gg] = *reinterpret_cast<const f32x4*>(sh_q + 64 * sub + 16 * h + 4 * gg);
    }
    char* xrow = xarea + cand * TOPKM_XROW;
    for (int t0 = 0; t0 < (S > 0 ? S : 1); t0 += 64) {            // (at least one round: surv2 is always written)
        const int t = t0 + cand;
        const unsigned long long key = t < S ? surv[t] : 0ull;
        const bool live = key != 0ull && topk_key_val(key) >= vmin;
        const uint32_t row = live ? topk_key_row(key) : 0u;
        const float* kr = a.keys + (int64_t)row * KEY_DIM + 4 * sub;
        f32x4 kc[4][4];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) kc[h][gg] = *reinterpret_cast<const f32x4*>(kr + 16 * (4 * h + gg));
        }
        // (a candidate's area row is written and read by its own 4 lanes only - one wave, whose LDS
        // operations execute in order: no barrier between rounds or between the writes and the reads)
        // piece (4 h + gg) of the row: quarter h, 64 bytes gg, this lane's 16 of them
#pragma unroll
        for (int h = 0; h < 4; ++h) {
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) *reinterpret_cast<f32x4*>(xrow + h * 272 + gg * 64 + sub * 16) = kc[h][gg];
        }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int h = 0; h < 4; ++h) {
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) kc[h][gg] = *reinterpret_cast<const f32x4*>(xrow + sub * 272 + h * 64 + gg * 16);
        }
        float acc = 0.f, v = 0.f;
        for (int step = 0; step < 4; ++step) {
            v = acc;
#pragma unroll
            for (int h = 0; h < 4; ++h) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
#pragma unroll
                    for (int gg = 0; gg < 4; ++gg) v = __builtin_fmaf(kc[h][gg][c], qc[h][gg][c], v);
                }
            }
            acc = topk_row_shr1(v);
        }
        if (sub == 3) surv2[t] = live ? topk_key(v, row) : 0ull;     // (t < TOPKM_CAP; entries past S: 0)
    }
}

// sum over the 4 lanes of a quad, in every lane of it (two DPP adds)
__device__ __forceinline__ int topk_sum4(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);     // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);     // quad_perm [2,3,0,1]
    return v;
}

// (after topk_merge_prefetch of the same query, and a workgroup barrier)
// Every instruction of this function is on the call's critical path and runs once: a wave64
// instruction takes >= 4 cycles, so ~500 of them are a microsecond (measured: a thread-serial rank
// over 256 heads alone took 7 us).  The usual case - up to 32 candidates reach the ranking - is
// therefore a short straight path: DPP reductions, ONE LDS atomic per wave, 8 lanes per candidate
// for the float32 chain and for its rank, results written by the lanes that hold them; four
// workgroup barriers and two global round trips (the lists, the candidates' key rows).
template <int L>
__device__ void topk_merge_query(char* lds, int64_t q, const TopkStreamArgs& a, int n_parts) {
    TopkMergeLds m(lds);
    const int p = threadIdx.x;                                        // blockDim.x == 256
    const int lane = p & 63, wave = p >> 6;
    const int k = a.k;
    unsigned long long kk[L];
    float dm = -INFINITY;
#pragma unroll
    for (int i = 0; i < L; ++i) kk[i] = 0ull;
    if (p < n_parts) {
#pragma unroll
        for (int i = 0; i < L; ++i) kk[i] = ld_agent(a.cand + (q * L + i) * n_parts + p);   // contiguous over the threads
        dm = __uint_as_float(ld_agent(reinterpret_cast<const uint32_t*>(a.dmax + q * n_parts + p)));
    }
    // ---- 1. a lower bound T of the 16th best value, from the list heads (each the maximum of a
    //      different row set): every wave finds its R largest heads - R rounds of a DPP
    //      max-reduction, one holder leaving per round.  R = 4 when all four waves hold lists: T =
    //      the smallest of the waves' 4th largest heads (sixteen heads are >= it; about the
    //      20th-25th largest head overall).  Banks so small that fewer workgroups streamed them:
    //      R = 16 and T = the 16th largest of the values handed in.
    const int R = n_parts > 192 ? 4 : MAX_TOPK;
    {
        uint32_t h = (uint32_t)(kk[0] >> 32);            // 0 = empty list
        uint32_t mx = 0u;
        for (int r = 0; r < R; ++r) {
            mx = topk_wave_umax(h);
            if (R != 4 && lane == 0) m.sh_head[wave * MAX_TOPK + r] = mx;
            const unsigned long long holders = __ballot(h == mx && mx != 0u);
            if (holders != 0ull && lane == __ffsll((long long)holders) - 1) h = 0u;   // one holder leaves
        }
        const uint32_t dmx = topk_wave_umax(topk_ordered_bits(dm));
        if (lane == 0) {
            if (R == 4) m.sh_head[wave] = mx;            // the wave's 4th largest head
            m.sh_d[wave] = topk_key_val((unsigned long long)dmx << 32);
        }
    }
    __syncthreads();
    uint32_t T;
    if (R == 4) {
        const uint32_t t01 = m.sh_head[0] < m.sh_head[1] ? m.sh_head[0] : m.sh_head[1];
        const uint32_t t23 = m.sh_head[2] < m.sh_head[3] ? m.sh_head[2] : m.sh_head[3];
        T = t01 < t23 ? t01 : t23;
    } else {
        T = 0u;
        const uint32_t v = m.sh_head[lane];              // 4 x 16 values: one per lane
        int rank = 0;                                    // unique ranks: ties by lane
        for (int i = 0; i < 64; ++i) {
            const uint32_t o = (uint32_t)__builtin_amdgcn_readlane((int)v, i);
            rank += (o > v || (o == v && i < lane)) ? 1 : 0;
        }
        const unsigned long long at15 = __ballot(rank == MAX_TOPK - 1);
        if (at15 != 0ull) T = (uint32_t)__builtin_amdgcn_readlane((int)v, __ffsll((long long)at15) - 1);
    }
    const float dall = fmaxf(fmaxf(m.sh_d[0], m.sh_d[1]), fmaxf(m.sh_d[2], m.sh_d[3]));
    float eps2 = 0.f;
    const bool approx = a.eps_rel > 0.f;        // prefilter form: the candidates' values are approximate
    if (approx) {          // (a bound, not a result: 1 % over the norm covers its rounding)
        const float nm = fmaxf(fmaxf(m.sh_n2[0], m.sh_n2[1]), fmaxf(m.sh_n2[2], m.sh_n2[3]));
        float r2 = 0.f;
        for (int i = 0; i < 4; ++i) { const float r = nm > 0.f ? m.sh_n2[i] / nm : 0.f; r2 += r * r; }
        eps2 = 2.f * a.eps_rel * 1.01f * (nm * sqrtf(r2)) * a.kmax;
    }
    if (eps2 > 0.f && T != 0u) T = topk_ordered_bits(topk_key_val((unsigned long long)T << 32) - eps2);
    // ---- 2. survivors: the entries >= T - the first c of a thread's sorted list - compacted into
    //      LDS; list position by list position while any lane still has one, the lanes of a wave
    //      taking consecutive places behind ONE LDS atomic per wave
    {
        int c = 0;
#pragma unroll
        for (int i = 0; i < L; ++i) c += (kk[i] != 0ull && (uint32_t)(kk[i] >> 32) >= T) ? 1 : 0;
        unsigned long long mask[L];
        int total = 0;
#pragma unroll
        for (int i = 0; i < L; ++i) {
            mask[i] = __ballot(c > i);
            total += __popcll(mask[i]);
        }
        if (total != 0) {                                      // wave-uniform
            int base = 0;
            if (lane == 0) base = atomicAdd(&m.sh_i[0], total);
            base = __builtin_amdgcn_readfirstlane(base);
#pragma unroll
            for (int i = 0; i < L; ++i) {
                if (mask[i] == 0ull) break;                    // (uniform; the lists are sorted: later masks are empty too)
                if (c > i)                                     // (at < TOPKM_CAP: every entry has a place)
                    m.surv[base + __popcll(mask[i] & ((1ull << lane) - 1ull))] = kk[i];
                base += __popcll(mask[i]);
            }
        }
    }
    __syncthreads();
    const int S = m.sh_i[0];
    // ---- 3. ranking and exactness of the short lists: if the largest value any lane, wave or
    //      workgroup let go could belong to the top k, the query goes to the brute-force path.
    bool unsafe;
    if (S <= 128) {
        // the usual case.  4 lanes per candidate, 64 candidates per round (two rounds beyond 64):
        // its float32 similarity (prefilter form: the candidates carry approximate values), then
        // its rank among all of them by counting, each lane of the quad against a quarter of
        // them; the quad that holds rank r writes result r.  The check compares the largest
        // dropped (approximate) value with the k-th exact one, 2 eps apart.
        const int sub = p & 3;
        const int n64 = S > 64 ? 2 : 1;
        if (approx) topk_exact_values(a, m.sh_q, lds + TOPKM_OFF_X, m.surv, m.surv2, S, -INFINITY);
        else if (sub == 3) {
            for (int rr = 0; rr < n64; ++rr) { const int t = 64 * rr + (p >> 2); m.surv2[t] = t < S ? m.surv[t] : 0ull; }
        }
        __syncthreads();
        for (int rr = 0; rr < n64; ++rr) {
            const unsigned long long mine = m.surv2[64 * rr + (p >> 2)];      // (0 past S)
            int r = 0;
            const ulonglong2* o = reinterpret_cast<const ulonglong2*>(m.surv2 + 16 * n64 * sub);
            for (int i = 0; i < 8 * n64; ++i) {
                const ulonglong2 oo = o[i];
                r += (oo.x > mine ? 1 : 0) + (oo.y > mine ? 1 : 0);
            }
            r = topk_sum4(r);
            if (sub == 0 && mine != 0ull && r < k) {
                a.oval[q * k + r] = topk_key_val(mine);
                a.oidx[q * k + r] = (int64_t)topk_key_row(mine) + a.row_offset;
                if (r == k - 1 && dall >= topk_key_val(mine) - eps2) m.sh_i[1] = 1;
            }
        }
        if (p >= S && p < k) {                                // (fewer than k rows exist, or the lists lost some)
            a.oval[q * k + p] = -INFINITY;
            a.oidx[q * k + p] = (int64_t)-1;
        }
        __syncthreads();
        // (nothing can have been dropped while fewer than k rows exist)
        unsafe = a.force_exact || m.sh_i[1] != 0 || (S < k && dall > -INFINITY);
        if (!unsafe) return;
    } else {
        // a crowd of near-equal similarities: ranked by (approximate) value first; prefilter form:
        // only those within 2 eps of the k-th best approximate value are recomputed, and ranked again
        topk_rank_into(m.surv, S, m.res);
        __syncthreads();
        const unsigned long long kth = m.res[k - 1];
        unsafe = a.force_exact || (kth != 0ull && dall >= topk_key_val(kth) - eps2) || (kth == 0ull && dall > -INFINITY);
        if (!unsafe && approx) {
            const float vmin = kth != 0ull ? topk_key_val(kth) - eps2 : -INFINITY;
            __syncthreads();                                   // (every thread has read res)
            if (p < MAX_TOPK) m.res[p] = 0ull;
            topk_exact_values(a, m.sh_q, lds + TOPKM_OFF_X, m.surv, m.surv2, S, vmin);
            __syncthreads();
            topk_rank_into(m.surv2, S, m.res);
            __syncthreads();
        }
    }
    if (unsafe) {                                              // (workgroup-uniform: every thread computed it from LDS)
        if (p == 0 && a.exact_count) atomicAdd(a.exact_count, 1);
        __syncthreads();                                       // (res is rewritten)
        topk_brute_force(a.keys, a.n_valid, m.sh_q, m.sh, m.res);
    }
    if (p < k) {
        const unsigned long long mm = m.res[p];
        a.oval[q * k + p] = mm ? topk_key_val(mm) : -INFINITY;
        a.oidx[q * k + p] = mm ? (int64_t)topk_key_row(mm) + a.row_offset : (int64_t)-1;
    }
}

// the merge as a launch of its own: one workgroup per query (batches larger than the stream grid)
template <int L>
__global__ __launch_bounds__(256, 2) void topk_merge_kernel(TopkStreamArgs a, int n_parts) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    topk_merge_prefetch<L>(smem, (int64_t)blockIdx.x, a);
    __syncthreads();
    topk_merge_query<L>(smem, (int64_t)blockIdx.x, a, n_parts);
}

}  // namespace range_hip
