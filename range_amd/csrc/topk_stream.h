// Small-batch top-k: the HBM-streaming form of the keys scan (range_topk_stream).
//
// For a handful of queries the scan is bound by streaming the N x 1 KB key rows, not by MFMA, and
// the 64-queries-per-workgroup decomposition of pass 1 wastes the machine.  Here the grid is
// PERSISTENT (one workgroup per CU, launched once): every WAVE streams its own 16-row key tiles
// through a wave-private LDS ring filled by LDS-DMA - no workgroup barrier in the tile loop -
// against G groups of 16 queries held in registers (G = 1 or 2 groups share one pass over the
// keys), and several passes run back to back in the one launch with the ring kept full across the
// pass boundary.  (One scan body, topk_stream_scan, in two forms of the key operand: float32 keys, and
// the bf16-key prefilter - what range_topk_stream runs by default.  The merge: topk_merge.h.)
//
// What makes the stream the only thing that takes time:
//  * the K fragments of a tile are read into registers at once, so the ring slot is free - and
//    its refill is on its way - BEFORE the tile's MFMAs and list work;
//  * the MFMAs are compiler builtins here (no 256-accumulator register pressure as in pass 2), so
//    hipcc pads their hazards and interleaves the list maintenance of the PREVIOUS tile's values
//    into the MFMA shadow of the current one (software pipeline of depth one);
//  * the per-lane candidate lists are SHORT (4 values per lane and group instead of 16): a wave
//    sees only N / 16 / n_waves tiles (6 for range_db_large), i.e. ~24 values per lane, so 16-deep
//    lists never saturate and every value costs a full insertion.  Exactness is kept by
//    bookkeeping: every lane tracks the largest value it ever let go (dmax), and so does every
//    merge on the way up; the final merge compares the largest dmax of a query with the k-th
//    value it found, and only if some dropped value could have belonged to the top-k - 5 of a
//    query's best 16 rows in the few rows ONE lane sees, or exact ties - recomputes that query by
//    brute force (bit-identical dot products: an MFMA chain is an fmaf chain in a fixed order).
//
// The way up, all inside the one launch (round 3; it used to be a second kernel of one 1024-thread
// workgroup per query over 4096 list entries, as long as the scan itself):
//   lane lists (4) -> the 4 lanes of a query: bitonic merge over shuffles -> wave list (8)
//   -> LDS -> the 4 waves of the workgroup: the same merge -> workgroup list (8) -> HBM,
//   written through (sc1), then one agent-scope ticket per workgroup;
//   the LAST min(B, n_wg) workgroups to take a ticket wait until all have (they are the ones
//   that wait least) and merge ONE query each from its n_wg x 8 entries (topk_merge_query): rank
//   by counting against the 16th largest list head, exactness check, float32 re-rank in the
//   prefilter form.  A batch with more queries than workgroups runs the same merge as a second
//   launch (topk_merge_kernel).
//
// Dot products are the same single dependent MFMA chain, in the same k order, as in the scan
// kernels of scan_common.h (qk_mfma): every kernel that forms a similarity gets the same float.
#pragma once
#include "async_err.h"
#include "engine_prims.h"
#include "scan_common.h"
#include "topk_lists.h"

namespace range_hip {

struct TopkStreamArgs {
    const float* keys;          // (n_pad,256)
    const float* ehat;          // (B,256)
    unsigned long long* cand;   // (n_groups * 16 queries, TOPKS_WL, n_wg) keys: entry i of every workgroup's list
                                // (sorted descending, 0 = empty) side by side, so that the merge reads coalesced
    float* dmax;                // (n_groups * 16 queries, n_wg) largest value dropped on the way
    int64_t B;
    int64_t n_valid;
    int32_t n_blocks;
    int32_t n_groups;           // ceil(B / 16)
    const void* keys_bf16;      // prefilter form: (n_tiles, 8 chunks, 64 lanes, 8) bf16, see keyfrag_kernel (topk_gemm.h)
    // ---- the merge (topk_merge_query), as the tail of the same launch when `fused`
    uint32_t* sync;             // TOPKS_SYNC_WORDS words (topks_tail): 8 arrival counters that only ever count up
    uint32_t sync_base[8];      // what the counters read when this launch starts (the host adds every fused
                                // launch's arrivals: nothing is zeroed, nothing a give-up could leave behind)
    uint32_t* err;              // host-mapped word (or null): set when a merging workgroup's bounded wait gave up
    int32_t debug_giveup;       // test hook: the merging workgroups behave as if their wait had expired
    int32_t fused;              // 1: the last min(B, n_wg) workgroups to arrive merge one query each
    int32_t k;
    int64_t row_offset;
    int32_t force_exact;
    int32_t* exact_count;
    float eps_rel, kmax;        // prefilter form: error bound of the approximate values (0: exact values)
    float* oval;                // (B,k)
    int64_t* oidx;              // (B,k)
};

constexpr int TOPKS_SG = 4;         // groups whose lists a wave carries through consecutive passes
constexpr int TOPKS_WL = 8;         // entries of a wave's and of a workgroup's list of one query
constexpr int TOPKS_RING_BYTES = 8 * BLK * KEY_DIM * 4;          // 128 KB of key tiles per workgroup
// behind the ring: the waves' lists of a supergroup (4 groups x 4 waves x 16 queries x 8 keys),
// their dmax, and the control words of the tail
constexpr int TOPKS_XL_BYTES = TOPKS_SG * 4 * 16 * TOPKS_WL * 8;
constexpr int TOPKS_XD_BYTES = TOPKS_SG * 4 * 16 * 4;
constexpr int TOPKS_LDS_BYTES = TOPKS_RING_BYTES + TOPKS_XL_BYTES + TOPKS_XD_BYTES + 64;
constexpr uint32_t TOPKS_SPIN_LIMIT = 1u << 21;   // polls (~1 us each) before a merging workgroup gives up

// Sorted (descending) list of the L best (value, row) a lane has met, plus the largest value it
// has let go.  push() is branch-free: the new value replaces the last entry if it is larger and
// bubbles up; whichever of the two does not stay goes into dmax.  Rows arrive in increasing
// order and the comparisons are strict, so among equal values the lower row stays ahead.
template <int L>
struct ShortList {
    float v[L];
    uint32_t row[L];
    float dmax;
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int i = 0; i < L; ++i) { v[i] = -INFINITY; row[i] = 0xFFFFFFFFu; }
        dmax = -INFINITY;
    }
    __device__ __forceinline__ void push(float x, uint32_t r) {
        const float last = v[L - 1];
        dmax = fmaxf(dmax, fminf(x, last));
        const bool ins = x > last;
        v[L - 1] = ins ? x : last;
        row[L - 1] = ins ? r : row[L - 1];
#pragma unroll
        for (int i = L - 1; i > 0; --i) {
            const bool up = v[i] > v[i - 1];
            const float hv = up ? v[i] : v[i - 1], lv = up ? v[i - 1] : v[i];
            const uint32_t hr = up ? row[i] : row[i - 1], lr = up ? row[i - 1] : row[i];
            v[i - 1] = hv; v[i] = lv; row[i - 1] = hr; row[i] = lr;
        }
    }
};

// The 4 lanes (j, g = 0..3) of a query each hold a sorted list of L keys: afterwards every one of
// them holds the sorted L best of the union.  Two rounds (lane ^ 16, lane ^ 32) of a bitonic
// merge: c[i] = max(a[i], b[L-1-i]) are the L largest of two descending lists and form a bitonic
// sequence, which log2(L) stages of compare-exchanges sort.  `drop` receives the largest key this
// LANE saw leave; the two lanes of a pair see the same pairs, but the first round of lanes (2,3)
// is invisible to lanes (0,1): the caller reduces `drop` over the 4 lanes (merge4_drop_max).
template <int L, int OFF>
__device__ __forceinline__ void merge4_short_round(unsigned long long (&k)[L], unsigned long long& drop) {
    unsigned long long p[L];
#pragma unroll
    for (int i = 0; i < L; ++i) p[i] = lane_xor_u64<OFF>(k[L - 1 - i]);
#pragma unroll
    for (int i = 0; i < L; ++i) {
        const bool up = k[i] > p[i];
        const unsigned long long lo = up ? p[i] : k[i];
        k[i] = up ? k[i] : p[i];
        drop = lo > drop ? lo : drop;
    }
#pragma unroll
    for (int d = L / 2; d >= 1; d >>= 1) {
#pragma unroll
        for (int i = 0; i < L; ++i) {
            if ((i & d) == 0) {
                const unsigned long long a = k[i], b = k[i + d];
                k[i] = a > b ? a : b;
                k[i + d] = a > b ? b : a;
            }
        }
    }
}
template <int L>
__device__ __forceinline__ void merge4_short(unsigned long long (&k)[L], unsigned long long& drop) {
    static_assert(L == 4 || L == 8 || L == 16, "power-of-two list");
    merge4_short_round<L, 16>(k, drop);
    merge4_short_round<L, 32>(k, drop);
}
// compare-exchange: afterwards a >= b
__device__ __forceinline__ void topk_cmpx(unsigned long long& a, unsigned long long& b) {
    const unsigned long long hi = a > b ? a : b, lo = a > b ? b : a;
    a = hi; b = lo;
}
// The 4 lanes (j, g) of a query each hold a sorted list of FOUR keys in k[0..3]: afterwards every
// one of them holds the sorted 8 best of the 16 in k[0..7].  Round 1 (lane ^ 16): two lists of 4 make
// a bitonic sequence of 8 - nothing is dropped, no padding moved around (the general merge4_short<8>
// on zero-padded lists costs 1.6x the instructions); round 2 (lane ^ 32): the 8 largest of two
// sorted lists of 8, as in merge4_short.
__device__ __forceinline__ void merge4_lists4_top8(unsigned long long (&k)[8], unsigned long long& drop) {
#pragma unroll
    for (int i = 0; i < 4; ++i) k[4 + i] = lane_xor_u64<16>(k[3 - i]);          // [own descending | partner ascending]
#pragma unroll
    for (int d = 4; d >= 1; d >>= 1) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if ((i & d) == 0) topk_cmpx(k[i], k[i + d]);
        }
    }
    unsigned long long p[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = lane_xor_u64<32>(k[7 - i]);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const bool up = k[i] > p[i];
        const unsigned long long lo = up ? p[i] : k[i];
        k[i] = up ? k[i] : p[i];
        drop = lo > drop ? lo : drop;
    }
#pragma unroll
    for (int d = 4; d >= 1; d >>= 1) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if ((i & d) == 0) topk_cmpx(k[i], k[i + d]);
        }
    }
}
// dmax of the merged list: the lanes' own dmax, and everything the merge dropped in ANY of the 4 lanes
__device__ __forceinline__ float merge4_drop_max(float dm, unsigned long long drop) {
    if (drop != 0ull) dm = fmaxf(dm, topk_key_val(drop));
    dm = fmaxf(dm, lane_xor16(dm));
    dm = fmaxf(dm, lane_xor32(dm));
    return dm;
}

// Agent-scope relaxed accesses (global_load / global_store ... sc1: past this CU's L1 and written
// through this XCD's L2): everything one workgroup hands to another inside the launch goes through
// these, and only these (guide: cdna_hip_programming.md, Guideline 16 - "every load sc1" form).
__device__ __forceinline__ void st_agent(unsigned long long* p, unsigned long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long ld_agent(const unsigned long long* p) {
    return __hip_atomic_load(const_cast<unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t ld_agent(const uint32_t* p) {
    return __hip_atomic_load(const_cast<uint32_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The first pass's query operand, loaded BEHIND THE COMPILER'S BACK: vector-memory results return
// in issue order, so a load hipcc counts, issued after the ring's first requests, makes hipcc wait
// with vmcnt(0) - for the whole ring (measured: the first tile's arithmetic started 6 us after the
// kernel, when all four tiles of every wave had landed).  These loads are issued FIRST, the ring's
// requests behind them, and topk_qwait<N> waits until at most the N younger operations (the
// ring's) are outstanding: the query is in registers one round trip after the kernel starts.
// (guide 5.7, form (ii): loads, then a wait statement naming every destination read-write.  The
// destinations are ACCUMULATOR registers: with vector-register destinations hipcc parked each
// loaded value in an accumulator register at once - a copy of data that had not landed yet; the
// generated code is checked for copies between the loads and the wait by tests/test_host_cpu.py.)
// PAIRS = false: d[i] = 16 bytes at p + 64 i; PAIRS = true: d[2 c], d[2 c + 1] = 32 bytes at p + 128 c
template <int I, int N, bool PAIRS>
struct TopkQLoad {
    static __device__ __forceinline__ void run(f32x4 (&d)[N], const char* p) {
        asm volatile("global_load_dwordx4 %0, %1, off offset:%2"
                     : "=a"(d[I]) : "v"(p), "i"(PAIRS ? (I >> 1) * 128 + (I & 1) * 16 : I * 64) : "memory");
        TopkQLoad<I + 1, N, PAIRS>::run(d, p);
    }
};
template <int N, bool PAIRS>
struct TopkQLoad<N, N, PAIRS> {
    static __device__ __forceinline__ void run(f32x4 (&)[N], const char*) {}
};
template <int VMCNT>
__device__ __forceinline__ void topk_qwait(f32x4 (&d)[16]) {
    asm volatile("s_waitcnt vmcnt(%16)"
                 : "+a"(d[0]), "+a"(d[1]), "+a"(d[2]), "+a"(d[3]), "+a"(d[4]), "+a"(d[5]), "+a"(d[6]), "+a"(d[7]),
                   "+a"(d[8]), "+a"(d[9]), "+a"(d[10]), "+a"(d[11]), "+a"(d[12]), "+a"(d[13]), "+a"(d[14]), "+a"(d[15])
                 : "i"(VMCNT) : "memory");
}

// End of a supergroup (its 4 query groups have seen all their passes): per group, the 4 lanes of
// a query merge their lists (bitonic, shuffles only) into the wave's 8 best; through LDS, wave w
// then merges the 4 waves' lists of group w into the workgroup's 8 best and writes them (sc1).
// Two workgroup barriers, outside the tile loop; the ring keeps streaming the next supergroup's
// first tiles meanwhile (its LDS is not touched here).
template <int L>
__device__ __forceinline__ void topks_publish(ShortList<L> (&lists)[TOPKS_SG], int sg, const TopkStreamArgs& a,
                                              char* smem, int lane, int wave, bool more) {
    static_assert(L == 4 && TOPKS_WL == 8, "merge4_lists4_top8");
    unsigned long long* wl = reinterpret_cast<unsigned long long*>(smem + TOPKS_RING_BYTES);
    float* wd = reinterpret_cast<float*>(smem + TOPKS_RING_BYTES + TOPKS_XL_BYTES);
    const int g = lane >> 4, j = lane & 15;
#pragma unroll
    for (int gi = 0; gi < TOPKS_SG; ++gi) {
        if (sg * TOPKS_SG + gi < a.n_groups) {
            unsigned long long kk[TOPKS_WL];
#pragma unroll
            for (int i = 0; i < TOPKS_WL; ++i) kk[i] = 0ull;
#pragma unroll
            for (int i = 0; i < L; ++i)
                kk[i] = lists[gi].row[i] != 0xFFFFFFFFu ? topk_key(lists[gi].v[i], lists[gi].row[i]) : 0ull;
            unsigned long long drop = 0ull;
            merge4_lists4_top8(kk, drop);
            const float dm = merge4_drop_max(lists[gi].dmax, drop);
            if (g == 0) {
                ulonglong2* o = reinterpret_cast<ulonglong2*>(wl + ((gi * 4 + wave) * 16 + j) * TOPKS_WL);
#pragma unroll
                for (int i = 0; i < TOPKS_WL; i += 2) o[i / 2] = make_ulonglong2(kk[i], kk[i + 1]);
                wd[(gi * 4 + wave) * 16 + j] = dm;
            }
        }
    }
    __syncthreads();
    const int grp = sg * TOPKS_SG + wave;
    if (grp < a.n_groups) {
        const ulonglong2* src = reinterpret_cast<const ulonglong2*>(wl + ((wave * 4 + g) * 16 + j) * TOPKS_WL);
        unsigned long long kk[TOPKS_WL];
#pragma unroll
        for (int i = 0; i < TOPKS_WL; i += 2) { const ulonglong2 t = src[i / 2]; kk[i] = t.x; kk[i + 1] = t.y; }
        unsigned long long drop = 0ull;
        merge4_short<TOPKS_WL>(kk, drop);
        const float dm = merge4_drop_max(wd[(wave * 4 + g) * 16 + j], drop);
        if (g == 0) {
            const int64_t qq = (int64_t)grp * 16 + j;
#pragma unroll
            for (int i = 0; i < TOPKS_WL; ++i) st_agent(a.cand + (qq * TOPKS_WL + i) * gridDim.x + blockIdx.x, kk[i]);
            st_agent(reinterpret_cast<uint32_t*>(a.dmax + qq * gridDim.x + blockIdx.x), __float_as_uint(dm));
        }
    }
    if (more) __syncthreads();       // (the list area is written again at the end of the next supergroup)
}

}  // namespace range_hip

#include "topk_merge.h"      // topk_merge_prefetch, topk_merge_query: what the tail below runs

namespace range_hip {

static_assert(TOPKM_LDS_BYTES <= TOPKS_RING_BYTES, "the tail's scratch fits the drained ring");

// End of the stream kernels.  Every workgroup takes a ticket once all its waves' list stores have
// completed; the last min(B, n_wg) to do so - per shard, below - wait for the rest and merge one
// query each.
//  * hand-off (guide, Guideline 16 / MI355X_MICROARCH.md visibility table, first row): payload
//    stores sc1, every storing wave waits vmcnt(0), workgroup barrier, ONE lane adds to a counter
//    (agent scope); the consumer polls the counters with sc1 loads, the other waves pass a
//    barrier that wave then joins, every load of the payload is sc1.  No fence on either side.
//  * the arrivals are counted in 8 SHARDS (blockIdx % 8, each counter on a line of its own): 256
//    adds to one word take ~3 us to drain (guide: fanin), 32 per word a fraction of that.  The
//    workgroups of shard s that arrive last merge the queries q = s (mod 8); a merging workgroup
//    polls all 8 counters (8 lanes, one load each).
//  * all workgroups of the grid are resident (one per CU, grid <= CUs), every one takes its
//    ticket BEFORE it may wait, and those that do not merge exit: the wait ends.  The spin is
//    bounded all the same; a workgroup that gives up marks its query's results invalid
//    (index -1, NaN) and sets the context's host-mapped error word: the host reports it at
//    its next entry or synchronising exit and runs the merge as a second launch from then on.
//  * the counters only ever count up: the host knows what they read when a launch starts
//    (a.sync_base: the sum of all earlier fused launches' arrivals, modulo 2^32) and tickets and
//    waits are differences to that base.  Nothing is zeroed - neither by the host in front of a
//    launch nor by the last workgroup to leave - so a workgroup that gave up leaves nothing behind
//    that a later launch could trip over (every workgroup of its launch still took its ticket).
//  * a merging workgroup loads its query (topk_merge_prefetch) before it waits.
constexpr int TOPKS_SYNC_STRIDE = 64;                          // words between shard counters (256 B)
constexpr int TOPKS_SYNC_SCRATCH = 8 * TOPKS_SYNC_STRIDE;      // host scratch behind the counters (the key-norm reduction)
constexpr int TOPKS_SYNC_WORDS = TOPKS_SYNC_SCRATCH + 16;
__device__ __forceinline__ void topks_tail(const TopkStreamArgs& a, char* smem) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // list stores done; the clamped prefetches past the end landed
    if (!a.fused) return;
    int* ctl = reinterpret_cast<int*>(smem + TOPKS_RING_BYTES + TOPKS_XL_BYTES + TOPKS_XD_BYTES);
    __syncthreads();
    const int n_wg = (int)gridDim.x;
    const int n_workers = a.B < (int64_t)n_wg ? (int)a.B : n_wg;
    const int shard = (int)(blockIdx.x & 7);
    const int shard_size = (n_wg - shard + 7) >> 3, shard_workers = (n_workers - shard + 7) >> 3;
    if (threadIdx.x == 0)
        ctl[0] = (int)(__hip_atomic_fetch_add(a.sync + TOPKS_SYNC_STRIDE * shard, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) -
                       a.sync_base[shard]);
    __syncthreads();
    const int local = ctl[0] - (shard_size - shard_workers);
    if (local < 0) return;
    const int64_t q = shard + 8 * local;
    if (q >= a.B) return;                  // (cannot happen while host and counters agree; never index past the batch)
    topk_merge_prefetch<TOPKS_WL>(smem, q, a);
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        const uint32_t need = lane < 8 ? (uint32_t)((n_wg - lane + 7) >> 3) : 0u;
        const uint32_t base = lane < 8 ? a.sync_base[lane] : 0u;
        int ok = 1;
        for (uint32_t spins = 0;; ++spins) {
            const uint32_t v = lane < 8 ? ld_agent(a.sync + TOPKS_SYNC_STRIDE * lane) - base : 0u;
            if (__ballot(v >= need) == ~0ull) break;
            if (spins > TOPKS_SPIN_LIMIT) { ok = 0; break; }
            __builtin_amdgcn_s_sleep(1);
        }
        if (a.debug_giveup) ok = 0;
        if (lane == 0) {
            ctl[1] = ok;
            if (!ok && a.err) __hip_atomic_store(a.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    __syncthreads();
    if (!ctl[1]) {
        if ((int)threadIdx.x < a.k) {
            a.oval[q * a.k + threadIdx.x] = __builtin_nanf("");
            a.oidx[q * a.k + threadIdx.x] = (int64_t)-1;
        }
        return;
    }
    topk_merge_query<TOPKS_WL>(smem, q, a, n_wg);
}

// ------------------------------------------------------------------------------------------------
// The scan: one body for both forms of the key operand.
//
// Prefilter on bf16 keys (TopksBf16Keys: the default of range_topk_stream; results identical to the
// float32 scan).  The float32 scan (TopksF32Keys) is not waiting for HBM at 16 queries: a wave spends
// its time in the 64 float32 MFMAs per tile and per query group.  The prefilter reads a bf16 copy of
// the keys (half the bytes) and forms APPROXIMATE similarities with 16 bf16 MFMAs per tile and group -
// the query to 16 significant bits (two bf16 planes), the key rounded to bf16 - so
//     |approx - exact| <= (2^-9 + 2^-17) |q| |k|   (+ 3e-5 of accumulation)  =: eps.
// A group's query operand is 64 registers; one or two groups share a pass over the keys.
// The lists, their dmax bookkeeping and the candidate layout are those of the float32 scan, on
// approximate values.  The merge then takes every candidate within 2 eps of the k-th best
// approximate value, recomputes ITS similarity with the float32 fmaf chain (= the MFMA chain of the
// float32 kernels, bit for bit) and ranks those: a row of the true top k cannot be missing (its
// approximate value is within eps of its exact one, and the k-th best approximate value within eps
// of the k-th best exact one) unless a list dropped it - which the dmax check, widened by the same
// 2 eps, detects and answers with the brute-force path as before.
//
// A form of the key operand says what topk_stream_scan does not know:
//   TILE_BYTES, DEPTH, OPS  a 16-row tile in the ring, ring slots per wave, LDS-DMA operations per tile
//   tiles, TILE_STRIDE      the tiles in global memory
//   issue                   a tile's OPS operations into a slot
//   PAIRS                   which 16 x 16 bytes of a query's row a lane holds (topk_q_f4)
//   QReg[QN], q_make, q_pin the lane's query operand, built from those 16 float4; made opaque
//   KReg[KN], k_lane_off,   a tile's K fragments: the lane's place in a slot, the reads from it
//     k_read                  into registers
//   dot, sched              the MFMA chain of one group; how the list work is dealt into its shadow

constexpr int TSB_TILE_BYTES = 8 * 1024;          // 16 rows x 256 bf16 in fragment order
constexpr int TSB_DEPTH = 4;                      // ring slots per wave (32 KB in flight per wave, as for float32 keys)
// eps / (|q| |k|): key rounding 2^-9 + query planes 2^-17 = 0.0019608, bf16 MFMA accumulation
// (512 terms) 3.1e-5, the float32 chain's own rounding (256 terms) 1.5e-5: 0.0020066 in the worst case
constexpr float TSB_EPS_REL = 0.0021f;

// float4 index, in a query's row, of the i-th of the 16 a lane of group g holds -
// PAIRS = false: Q[j][16 i + 4 g .. +3]; PAIRS = true: Q[j][32 c + 8 g .. +7] in 2 c, 2 c + 1 (TopkQLoad)
template <bool PAIRS>
__device__ __forceinline__ constexpr int topk_q_f4(int i, int g) {
    return PAIRS ? 8 * (i >> 1) + 2 * g + (i & 1) : 4 * i + g;
}

// float32 keys: a tile is 16 rows of 1 KB; lane (j, g) holds Q[j][16 s + 4 g .. +3] as it is
struct TopksF32Keys {
    static constexpr uint32_t TILE_BYTES = BLK * KEY_DIM * 4;
    static constexpr int DEPTH = 2, OPS = 16;
    static constexpr bool PAIRS = false;
    static constexpr int QN = 16, KN = 16;
    typedef f32x4 QReg;
    typedef f32x4 KReg;
    KAddr kaddr;
    __device__ __forceinline__ explicit TopksF32Keys(int lane) {
        kaddr.init(lane);
        // (four registers, as such: hipcc otherwise re-forms one of them from its parts inside the
        // tile loop, and the two-group kernel has no register to hold a part in)
#pragma unroll
        for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(kaddr.b[i]));
    }
    static __device__ __forceinline__ int k_lane_off(int) { return 0; }       // (kaddr: a row per lane, swizzled)
    static constexpr int TILE_STRIDE = BLK * KEY_DIM;                         // in elements of tiles()
    static __device__ __forceinline__ const float* tiles(const TopkStreamArgs& a) { return a.keys; }
    // 16 DMA instructions (4 groups of 4 rows, swizzled source: chunk c of row R lands at chunk
    // position c ^ R, which makes the ds_read_b128 of k_read conflict-free)
    static __device__ __forceinline__ void issue(const float* src, uint32_t dst, int lane) {
#pragma unroll
        for (int gr = 0; gr < 4; ++gr) {
            dma_group_begin(dst + gr * 4096);
#pragma unroll
            for (int i4 = 0; i4 < 4; ++i4)
                // (non-temporal: a key tile is read by exactly one wave per pass - measured 1 us
                // per 16-query launch and 3 us per four passes faster than the default policy)
                dma_b128_q_nt(src + gr * 4 * KEY_DIM, (uint32_t)((lane ^ (4 * gr + i4)) << 4), i4);
        }
    }
    static __device__ __forceinline__ void q_make(QReg (&q)[QN], const f32x4 (&raw)[16]) {
#pragma unroll
        for (int s = 0; s < 16; ++s) q[s] = raw[s];
    }
    static __device__ __forceinline__ void q_pin(QReg (&q)[QN]) {
#pragma unroll
        for (int s = 0; s < 16; ++s) asm volatile("" : "+v"(q[s]));
    }
    __device__ __forceinline__ void k_read(KReg (&kf)[KN], const char* kt) const {
#pragma unroll
        for (int s = 0; s < 16; ++s) kf[s] = *reinterpret_cast<const f32x4*>(kt + kaddr.b[s & 3] + 256 * (s >> 2));
    }
    static __device__ __forceinline__ f32x4 dot(const KReg (&kf)[KN], const QReg (&q)[QN]) {
        f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            c = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[s].x, q[s].x, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[s].y, q[s].y, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[s].z, q[s].z, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[s].w, q[s].w, c, 0, 0, 0);
        }
        return c;
    }
    static __device__ __forceinline__ void sched() {
        constexpr int VALU_PER_MFMA = 4;
#pragma unroll
        for (int m = 0; m < 64; ++m) {
            __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);    // 1 MFMA
            __builtin_amdgcn_sched_group_barrier(0x2, VALU_PER_MFMA, 0);
        }
    }
};

// bf16 fragments (keyfrag_kernel): a tile is 8 KB, contiguous in fragment order; the B operand of lane
// (n = query j, kg = g) is Q[j][32 c + 8 g + 0..7], chunk c, as two bf16 planes (q = q_h + q_m to
// 2^-17): q[c] = q_h, q[8 + c] = q_m
struct TopksBf16Keys {
    static constexpr uint32_t TILE_BYTES = TSB_TILE_BYTES;
    static constexpr int DEPTH = TSB_DEPTH, OPS = 8;
    static constexpr bool PAIRS = true;
    static constexpr int QN = 16, KN = 8;
    typedef u32x4 QReg;
    typedef u32x4 KReg;
    __device__ __forceinline__ explicit TopksBf16Keys(int) {}
    static __device__ __forceinline__ int k_lane_off(int lane) { return lane * 16; }
    static constexpr int TILE_STRIDE = TSB_TILE_BYTES;
    static __device__ __forceinline__ const char* tiles(const TopkStreamArgs& a) { return reinterpret_cast<const char*>(a.keys_bf16); }
    // 8 LDS-DMA operations (two groups of four)
    static __device__ __forceinline__ void issue(const char* src, uint32_t dst, int lane) {
#pragma unroll
        for (int gr = 0; gr < 2; ++gr) {
            dma_group_begin(dst + gr * 4096);
#pragma unroll
            for (int i4 = 0; i4 < 4; ++i4) dma_b128_q_nt(src + gr * 4096, (uint32_t)(lane << 4), i4);
        }
    }
    static __device__ __forceinline__ void q_make(QReg (&q)[QN], const f32x4 (&raw)[16]) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const f32x4 v0 = raw[2 * c], v1 = raw[2 * c + 1];
            const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                uint32_t h, m;
                float ra, rb;
                split2(v[2 * e], v[2 * e + 1], h, m, ra, rb);
                q[c][e] = h; q[8 + c][e] = m;
            }
        }
    }
    static __device__ __forceinline__ void q_pin(QReg (&q)[QN]) {
#pragma unroll
        for (int c = 0; c < 8; ++c) asm volatile("" : "+v"(q[c]), "+v"(q[8 + c]));
    }
    __device__ __forceinline__ void k_read(KReg (&kf)[KN], const char* kt) const {
#pragma unroll
        for (int c = 0; c < 8; ++c) kf[c] = *reinterpret_cast<const u32x4*>(kt + c * 1024);
    }
    static __device__ __forceinline__ f32x4 dot(const KReg (&kf)[KN], const QReg (&q)[QN]) {
        f32x4 c0 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 8; ++c)        // small terms first
            c0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kf[c]), __builtin_bit_cast(bf16x8, q[8 + c]), c0, 0, 0, 0);
#pragma unroll
        for (int c = 0; c < 8; ++c)
            c0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kf[c]), __builtin_bit_cast(bf16x8, q[c]), c0, 0, 0, 0);
        return c0;
    }
    static __device__ __forceinline__ void sched() {}      // (hipcc's own interleaving)
};

// 4 waves per workgroup, each with a ring of DEPTH tiles (4 * DEPTH * TILE_BYTES of LDS = 128 KB).
// Per-wave stamps (float32 keys) show that with 4 waves x 2 tiles a wave never waits for a
// tile once the first has landed: over a pass it spends 7.9 us in arithmetic, 2.4 us issuing
// LDS-DMA and 0 us waiting.  8 waves x 1 tile (two waves per SIMD) was measured for the 1-group
// kernel: 21.4 us instead of 21.6 at 16 queries, but 37.3 / 70 us instead of 36.2 / 63.6 at 2 / 4
// passes - so the instantiation is 4 x 2 (and the workgroup-level merge counts on 4 waves).
template <class Op, int G, int L>
__device__ __forceinline__ void topk_stream_scan(const TopkStreamArgs& a, char* smem) {
    constexpr int NW = 4, DEPTH = Op::DEPTH, OPS = Op::OPS;
    constexpr uint32_t TILE = Op::TILE_BYTES;
    static_assert(NW * DEPTH * TILE == TOPKS_RING_BYTES, "the waves' rings are the ring area");
    constexpr int PPS = TOPKS_SG / G;                          // passes per supergroup
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, j = lane & 15;
    const uint32_t lds0 = (uint32_t)(uintptr_t)RANGE_LPTR(smem) + wave * DEPTH * TILE;
    const char* my = smem + wave * DEPTH * TILE + Op::k_lane_off(lane);      // this lane's view of the wave's ring

    const int n_waves = gridDim.x * NW;
    // (wave-major ids: the waves that get one tile more than the rest - the first n_blocks mod
    // n_waves ids - are then spread one per CU instead of filling whole workgroups)
    const int w_id = wave * gridDim.x + blockIdx.x;
    // this wave's tiles: w_id, w_id + n_waves, ... once per pass (T per pass, the last one of a
    // pass possibly past the bank: fetched as the bank's last tile, never consumed).  (Dealing a
    // workgroup's tiles to its waves through a counter in LDS was measured: the spread of the
    // waves' finishing times is between XCDs and CUs, not inside a workgroup, and did not shrink.)
    const int T = (a.n_blocks + n_waves - 1) / n_waves;        // tiles per wave and pass
    const int n_pass = (a.n_groups + G - 1) / G;               // passes over the keys, all supergroups
    const int n_sg = (a.n_groups + TOPKS_SG - 1) / TOPKS_SG;
    const int total = n_pass * T;                              // this wave's tile sequence
    const int last = a.n_blocks - 1;
    // Sequence positions past the end fetch the bank's last tile again - never consumed - so
    // that every wait below is a constant.
    auto issue_seq = [&](int k) __attribute__((always_inline)) {
        const int i = k < total ? k % T : T - 1;
        const int tile = w_id + i * n_waves;
        Op::issue(Op::tiles(a) + (int64_t)(tile < last ? tile : last) * Op::TILE_STRIDE, lds0 + (k % DEPTH) * TILE, lane);
    };
    // The first pass's query rows first, the ring's first requests behind them (why, and why by
    // hand: at TopkQLoad)
    f32x4 qraw0[G][16];
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
        const int grp = min(gi, a.n_groups - 1);
        const int64_t q = (int64_t)grp * 16 + j;
        TopkQLoad<0, 16, Op::PAIRS>::run(
            qraw0[gi], reinterpret_cast<const char*>(a.ehat + (q < a.B ? q : a.B - 1) * KEY_DIM + 4 * topk_q_f4<Op::PAIRS>(0, g)));
    }
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) issue_seq(d);

    const Op op(lane);
    uint32_t prow[4];
    lane_rows(prow, g);
    const uint32_t n_valid32 = (uint32_t)a.n_valid;

    int k = 0;                                                 // position in the tile sequence
    for (int sg = 0; sg < n_sg; ++sg) {
        // the lists of a supergroup's 4 query groups live in registers through its passes and
        // are merged once, at its end: no merge work at a pass boundary
        ShortList<L> lists[TOPKS_SG];
#pragma unroll
        for (int gi = 0; gi < TOPKS_SG; ++gi) lists[gi].init();
#pragma unroll
        for (int ps = 0; ps < PPS; ++ps) {
            const int grp0 = (sg * PPS + ps) * G;                         // first group of this pass
            if (grp0 < a.n_groups) {
                typename Op::QReg qf[G][Op::QN];                          // this pass's groups
#pragma unroll
                for (int gi = 0; gi < G; ++gi) {
                    f32x4 qraw[16];
                    if (ps == 0 && sg == 0) {
                        // (issued in front of the ring's DEPTH x OPS requests, and of the later group's loads)
                        if (gi == 0 && G == 2) topk_qwait<DEPTH * OPS + 16>(qraw0[0]);
                        else topk_qwait<DEPTH * OPS>(qraw0[gi]);
#pragma unroll
                        for (int i = 0; i < 16; ++i) qraw[i] = qraw0[gi][i];
                    } else {
                        const int grp = min(grp0 + gi, a.n_groups - 1);
                        const int64_t q = (int64_t)grp * 16 + j;
                        const f32x4* rowp =
                            reinterpret_cast<const f32x4*>(a.ehat + (q < a.B ? q : a.B - 1) * KEY_DIM);
#pragma unroll
                        for (int i = 0; i < 16; ++i) qraw[i] = rowp[topk_q_f4<Op::PAIRS>(i, g)];
                    }
                    Op::q_make(qf[gi], qraw);
                }
                // (ordinary loads that hipcc counts: "using" them here puts its wait for them in
                // front of the tile loop - at their first use inside it, it would be a vmcnt(0)
                // that drains the hand-counted LDS-DMA ring every iteration)
#pragma unroll
                for (int gi = 0; gi < G; ++gi) Op::q_pin(qf[gi]);
                // values of the previous tile, pushed while the current tile's MFMAs run (the
                // first round pushes -inf: a no-op)
                f32x4 prev[G];
#pragma unroll
                for (int gi = 0; gi < G; ++gi) prev[gi] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                uint32_t prev_row0 = 0;
                auto push_prev = [&](int gi) __attribute__((always_inline)) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const uint32_t row = prev_row0 + prow[r];
                        // (pad rows exist in the bank's last tile only; a compare is cheaper than a branch)
                        const float x = row < n_valid32 ? prev[gi][r] : -INFINITY;
                        lists[ps * G + gi].push(x, row);
                    }
                };

                for (int i = 0; i < T; ++i, ++k) {
                    const int tile = w_id + i * n_waves;
                    // tile k has landed when at most the OPS operations of each younger tile are outstanding
                    asm volatile("s_waitcnt vmcnt(%0)" ::"i"((DEPTH - 1) * OPS) : "memory");
                    typename Op::KReg kf[Op::KN];
                    op.k_read(kf, my + (k % DEPTH) * TILE);
                    // the slot is free once these reads have returned: refill it before the arithmetic
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                    for (int s = 0; s < Op::KN; ++s) asm volatile("" : "+v"(kf[s]));
                    issue_seq(k + DEPTH);
                    if (tile >= a.n_blocks) continue;      // (the ragged last round of a pass)
                    f32x4 acc[G];
#pragma unroll
                    for (int gi = 0; gi < G; ++gi) {
                        acc[gi] = Op::dot(kf, qf[gi]);
                        // list maintenance of the PREVIOUS tile's values of this group:
                        // independent of the chain above, placed into its shadow
                        push_prev(gi);
                        Op::sched();
                    }
#pragma unroll
                    for (int gi = 0; gi < G; ++gi) prev[gi] = acc[gi];
                    prev_row0 = (uint32_t)tile * BLK;
                }
#pragma unroll
                for (int gi = 0; gi < G; ++gi) push_prev(gi);
            }
        }
        topks_publish<L>(lists, sg, a, smem, lane, wave, sg + 1 < n_sg);
    }
    topks_tail(a, smem);
}

template <int G, int L, int NW, int DEPTH>
__global__ __launch_bounds__(NW * 64, NW / 4) void topk_stream_kernel(TopkStreamArgs a) {
    static_assert(TOPKS_SG % G == 0, "groups per pass must divide the supergroup");
    static_assert(NW == 4 && DEPTH == 2, "128 KB of key tiles per workgroup, one wave per group in the workgroup merge");
    static_assert(DEPTH == TopksF32Keys::DEPTH, "the ring depth is the operand form's");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    topk_stream_scan<TopksF32Keys, G, L>(a, smem);
}

template <int G, int L>
__global__ __launch_bounds__(256, 1) void topk_stream_bf16_kernel(TopkStreamArgs a) {
    static_assert(TOPKS_SG % G == 0, "groups per pass must divide the supergroup");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    topk_stream_scan<TopksBf16Keys, G, L>(a, smem);
}

}  // namespace range_hip

// A plain one-launch streaming read of the same bytes the top-k scan streams (range_stream_read_timed,
// topk_host.h): 16-byte non-temporal loads, 8 in flight per thread, 1 024 workgroups; the xor of everything
// read goes to one word per workgroup so that the loads stay.
// (extern "C": the symbol is the plain name)
extern "C" __global__ __launch_bounds__(256) void stream_read_kernel(const range_hip::u32x4* __restrict__ p, int64_t n16, int passes,
                                                          uint32_t* __restrict__ sink) {
    using range_hip::u32x4;
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
