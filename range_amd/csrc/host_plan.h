// Pure host arithmetic of the engine - launch plans, the encoder's slot plan, recurrence
// tables, weight packing - free of any HIP dependency, so that the same code the library runs is
// also compiled with g++ under AddressSanitizer / UndefinedBehaviorSanitizer / ThreadSanitizer on
// the CPU (tests/native/host_sanitize.cpp, tests/test_host_cpu.py).  GPU sanitizers are not
// available on the target pool; this is the part of the C-ABI shim that can be sanitised.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace range_host {

// Number of bank splits.  Workgroups of both scan kernels are equal-cost, so the chip runs them
// in near lock-step "rounds" of n_cu * wg_per_cu workgroups: pick the split count whose last
// round is best filled (e.g. 157 query tiles x 13 splits = 2041 workgroups = 7.97 rounds of 256),
// preferring fewer splits (less partial-result traffic) on near-ties.  wg_per_cu: 1 for pass 2
// (512 registers, 129 KB LDS), 4 for pass 1 (33 KB LDS, <= 128 VGPRs).
inline int choose_splits(int n_qtiles, int n_blocks, int n_cu, int wg_per_cu, int max_splits,
                         double split_cost = 0.002) {
    const double slots = (double)n_cu * wg_per_cu;
    const int cap = std::max(1, std::min(max_splits, n_blocks / 4));   // >= 4 blocks per split
    // small batches: first of all give every slot a workgroup
    const int ns_min = std::min(cap, (int)std::ceil(slots / n_qtiles));
    int best = ns_min;
    double best_score = -1e9;
    for (int ns = ns_min; ns <= cap; ++ns) {
        const double total = (double)n_qtiles * ns;
        const double rounds = std::ceil(total / slots);
        double score = total / (rounds * slots);            // fill of the rounds
        if (rounds < 4) score *= 0.85 + 0.0375 * rounds;    // few rounds: ragged finish hurts more
        score -= split_cost * (ns - ns_min);                // partial-result traffic
        if (score > best_score) { best_score = score; best = ns; }
        if (ns - ns_min > 64) break;
    }
    return best;
}

// Stream-K partition of pass 2 (scan_common.h: SlabMap, pass2.h: SegWalk; round 5): U units in order are cut
// into G contiguous, near-equal ranges [start(w), start(w + 1)); owner(u) is the range a unit falls in.
// The kernel walks by `start`, the reduction finds a query tile's parts by `owner`: both are these
// functions (compiled for the device too: RANGE_HD), and tests/native/host_sanitize.cpp checks that they
// agree for every unit.
#ifndef RANGE_HD
#if defined(__HIPCC__)
#define RANGE_HD __host__ __device__ __forceinline__
#else
#define RANGE_HD inline
#endif
#endif
RANGE_HD int64_t sk_start(int64_t w, int64_t U, int64_t G) { return (w * U) / G; }
RANGE_HD int64_t sk_owner(int64_t u, int64_t U, int64_t G) { return ((u + 1) * G - 1) / U; }
// first of n items that part i of n_parts takes (parts: contiguous, near-equal ranges; part i ends where
// part i + 1 begins): the bank blocks of a split, a chunk, a stream-K column or a workgroup
RANGE_HD int part_begin(int i, int n, int n_parts) { return (int)(((int64_t)i * n) / n_parts); }
RANGE_HD int sk_col_begin(int c, int n_blocks, int n_cols) { return part_begin(c, n_blocks, n_cols); }   // first block of bank column c

// Small-batch encoder: workgroups per 16-query tile = column parts S (a power of two, parts of
// 64 .. 512 columns: the widths a kernel exists for) x K parts KP (ranges of at least 3 of the
// first layer's slots).  Every workgroup gets its own CU (tiles * S * KP <= n_cu); K parts come
// first - a column part re-generates all the features of its K range, a K part generates only
// its share.  1 x 1: no split.
inline void choose_encoder_split(int n_cu, int n_slots, int H, long long tiles, int& S, int& KP) {
    S = 1;
    KP = 1;
    const int kp_max = std::max(1, std::min(7, n_slots / 3));
    for (int kp = 1; kp <= kp_max; ++kp)
        for (int s2 = 1; s2 <= 8; s2 *= 2) {
            const int part = H / s2;
            if (H % s2 || !(part == 64 || part == 128 || part == 256 || part == 512)) continue;
            if (tiles * s2 * kp > n_cu) continue;
            if (s2 * kp > S * KP || (s2 * kp == S * KP && kp > KP)) { S = s2; KP = kp; }
        }
}

// The encoder's first-layer K order: the L*L spherical-harmonic features permuted into "slots"
// (slot 0 = order 0; slot s >= 1 = orders {s, L-s}, or {s} when s == L-s), every slot padded to
// whole k-step pairs (8 features).  perm: padded position -> feature index l*l+l+m, or -1.
struct EncoderPlan {
    std::vector<int> perm;
    std::vector<int32_t> slot_base;   // [n_slots + 1]
    int n_slots = 0, n_rounds = 0, max_round = 0;
};

inline bool build_encoder_plan(int L, int slots_per_round, EncoderPlan& p) {
    std::vector<int> slot_m_a, slot_m_b;
    slot_m_a.push_back(0);
    slot_m_b.push_back(-1);
    for (int s = 1; s <= L - s && s < L; ++s) {
        slot_m_a.push_back(s);
        slot_m_b.push_back(L - s > s ? L - s : -1);
    }
    p.n_slots = (int)slot_m_a.size();
    p.slot_base.assign(p.n_slots + 1, 0);
    p.perm.clear();
    for (int s = 0; s < p.n_slots; ++s) {
        p.slot_base[s] = (int32_t)p.perm.size();
        for (int c2 = 0; c2 < 2; ++c2) {
            const int m = c2 == 0 ? slot_m_a[s] : slot_m_b[s];
            if (m < 0) break;
            for (int l = m; l < L; ++l) {
                if (m == 0) p.perm.push_back(l * l + l);
                else { p.perm.push_back(l * l + l + m); p.perm.push_back(l * l + l - m); }
            }
        }
        while (p.perm.size() % 8) p.perm.push_back(-1);   // whole k-step pairs (8 features)
    }
    p.slot_base[p.n_slots] = (int32_t)p.perm.size();
    // every feature exactly once
    std::vector<char> seen((size_t)L * L, 0);
    int cnt = 0;
    for (int f : p.perm)
        if (f >= 0) {
            if (f >= L * L || seen[f]) return false;
            seen[f] = 1;
            ++cnt;
        }
    if (cnt != L * L) return false;
    p.n_rounds = (p.n_slots + slots_per_round - 1) / slots_per_round;
    p.max_round = 0;
    for (int r = 0; r < p.n_rounds; ++r) {
        const int s1 = std::min((r + 1) * slots_per_round, p.n_slots);
        p.max_round = std::max(p.max_round, p.slot_base[s1] - p.slot_base[r * slots_per_round]);
    }
    return true;
}

// Three-term recurrence on fully normalised associated Legendre functions: q(l,m) =
// a(l,m) * (x q(l-1,m) - b(l,m) q(l-2,m)); coefA = a, coefB = a*b at [l*L+m]; seedc[m] = the chain
// seed's constant with the reference's convention folded in (analytic: pi-scaled m = 0, no
// Condon-Shortley sign; closed-form: orthonormal m = 0, sign kept).
inline void recurrence_tables(int L, bool analytic, std::vector<double>& coefA, std::vector<double>& coefB,
                              std::vector<double>& seedc) {
    coefA.assign((size_t)L * L, 0.0);
    coefB.assign((size_t)L * L, 0.0);
    seedc.assign(L, 0.0);
    const double PI = 3.14159265358979323846;
    double cm = std::sqrt(1.0 / (4.0 * PI));
    for (int m = 0; m < L; ++m) {
        if (m > 0) cm *= std::sqrt((2.0 * m + 1.0) / (2.0 * m));
        double scale;
        if (m == 0) scale = analytic ? PI : 1.0;
        else scale = std::sqrt(2.0) * ((!analytic && (m & 1)) ? -1.0 : 1.0);
        seedc[m] = cm * scale;
        for (int l = m + 1; l < L; ++l) {
            if (l == m + 1) {
                coefA[(size_t)l * L + m] = std::sqrt(2.0 * m + 3.0);
                coefB[(size_t)l * L + m] = 0.0;
            } else {
                const double a = std::sqrt((4.0 * l * l - 1.0) / ((double)l * l - (double)m * m));
                const double b = std::sqrt((((double)l - 1.0) * (l - 1.0) - (double)m * m) /
                                           (4.0 * (l - 1.0) * (l - 1.0) - 1.0));
                coefA[(size_t)l * L + m] = a;
                coefB[(size_t)l * L + m] = a * b;
            }
        }
    }
}

// The hidden width the encoder kernels run a checkpoint's `capacity` at: kernels exist for multiples
// of 64 up to 512, and for 768 and 1024; any other width up to 1024 runs as the next of those with
// zero-padded weights (a padded unit is sin(w0 (0 . x + 0)) = 0 feeding zero weights: every product
// it adds is an exact +0.0, the unpadded network's result bit for bit).  0: unsupported.
inline int kernel_hidden_width(int hidden) {
    if (hidden < 1 || hidden > 1024) return 0;
    return hidden <= 512 ? (hidden + 63) / 64 * 64 : (hidden <= 768 ? 768 : 1024);
}

// (n_out x k_in) row-major -> (n_pad x k_pad), the new rows and columns zero
inline std::vector<double> pad_weights(const double* W, int n_out, int k_in, int n_pad, int k_pad) {
    std::vector<double> P((size_t)n_pad * k_pad, 0.0);
    for (int r = 0; r < n_out; ++r)
        std::copy(W + (size_t)r * k_in, W + (size_t)(r + 1) * k_in, P.begin() + (size_t)r * k_pad);
    return P;
}

// Query ranges of the numpy contract's pass 2 (range_forward_host): the batch in parts, the tail parts
// of the given nominal sizes (the last ones shortest: their copies are what the caller waits for), cuts
// rounded UP to a query tile, never past the batch and never backwards - whatever `tail` holds.
// Returns the cut positions, first 0 and last B.
inline std::vector<int64_t> host_part_cuts(int64_t B, const std::vector<int64_t>& tail, int64_t tile) {
    std::vector<int64_t> cuts{0};
    int64_t rest = 0;
    for (auto v : tail) rest += v;
    if (rest < B) {
        int64_t at = B - rest;
        for (auto v : tail) {
            const int64_t cut = std::min<int64_t>(B, (at + tile - 1) / tile * tile);
            if (cut > cuts.back()) cuts.push_back(cut);
            at += v;
        }
        if (cuts.back() == B) cuts.pop_back();
    }
    cuts.push_back(B);
    return cuts;
}

// Weights (n_out, k_in) row-major -> MFMA B-fragment order, two k-steps per 16-byte lane element:
//   [((ntile*kpairs + kpair)*64 + lane)*2 + e] = W[ntile*16 + (lane&15)][kperm[kpair*8 + 4e + (lane>>4)]]
// (kperm: padded position -> column or -1 for a zero pad; null: identity).
inline std::vector<double> pack_weights(const double* W, int n_out, int k_in, const std::vector<int>* kperm,
                                        int Kpad) {
    const int kp = Kpad / 8, nt = n_out / 16;
    std::vector<double> out((size_t)nt * kp * 128);
    for (int t = 0; t < nt; ++t)
        for (int s = 0; s < kp; ++s)
            for (int ln = 0; ln < 64; ++ln)
                for (int e = 0; e < 2; ++e) {
                    const int n = t * 16 + (ln & 15);
                    const int kk = s * 8 + 4 * e + (ln >> 4);
                    const int k = kperm ? (*kperm)[kk] : kk;
                    out[(((size_t)t * kp + s) * 64 + ln) * 2 + e] = k >= 0 ? W[(size_t)n * k_in + k] : 0.0;
                }
    return out;
}

// ---- Launch plans: every number a launch site of range_hip.hip's parts needs - which kernel variant, grid,
// the argument fields derived from geometry, workspace sizes - as pure functions of integers and
// switches.  The *_host.h parts allocate, fill pointers and launch what a plan says;
// tests/native/host_sanitize.cpp asks the plans the cases the comments below state.

// Integer constants of the kernel headers that the plans need.  The kernel headers keep the only
// definition of each; engine_ctx.h fills this struct from them once (PLAN_CONSTS).
struct PlanConsts {
    int qtile, blk, val_dim, max_topk, p1_wg_per_cu;   // engine_prims.h: QTILE, BLK, VAL_DIM, MAX_TOPK; pass1.h: P1_WG_PER_CU
    int enc_qtile;                                     // encoder_kernel.h: ENC_QTILE
    int topks_wl;                                      // topk_stream.h: TOPKS_WL
    int tg_qblock, tg_wg_per_cu, tg_cap_l;             // topk_gemm.h: TG_QBLOCK, TG_WG_PER_CU, TG_CAP_L
};

// Small batches (fewer 16-query tiles than half the CUs): the first layer - 70 % of the weights
// a workgroup streams - is split over S column parts per tile on S times as many workgroups
// (encoder_l1_part_kernel), the rest follows per tile (encoder_rest_kernel).  One workgroup's
// serial chain over all weights takes 0.28 ms whatever the batch; this pair takes about half.
// the first layer's part kernels exist for parts of 64, 128, 256 and 512 columns
inline bool split_width_ok(int H, int S) {
    const int part = H / S;
    return H % S == 0 && (part == 64 || part == 128 || part == 256 || part == 512);
}

// The small-batch encoder on `tiles` 16-query tiles with S x KP workgroups each.
struct EncSplitPlan {
    int tiles = 0, S = 1, KP = 1;
    int part_cols = 0;          // first-layer columns of a part (H / S); the kernels are instantiated per part_cols / 64
    int grid = 0;               // tiles * S * KP workgroups of the first (or only) launch
    bool one_launch = false;    // encoder_tile_kernel: all phases in one persistent launch
    int S2 = 1;                 // separate launches: second layer over S2 column parts per tile (1: inside the last kernel)
    int n_parts2 = 0, part2_cols = 0;   // second-layer parts (one_launch or S2 > 1)
    int rest_from = 0;          // EncArgs::rest_from of the last phase / launch
    size_t h1_doubles = 0;      // partial sums of the first layer: KP * tiles * 16 * H
    size_t tile_doubles = 0;    // a (tiles * 16, H) activation buffer (h1a, h2)
};

inline EncSplitPlan plan_encoder_split(int n_cu, int H, int n_layers, bool enc_fused, int64_t B, int S, int KP) {
    EncSplitPlan p;
    const int tiles = (int)((B + 15) / 16);
    p.tiles = tiles;
    p.S = S;
    p.KP = KP;
    p.part_cols = H / S;
    p.grid = tiles * S * KP;
    p.h1_doubles = (size_t)KP * tiles * 16 * H;
    p.tile_doubles = (size_t)tiles * 16 * H;
    // up to 32 tiles (512 queries): all phases in ONE launch (encoder_tile_kernel), every tile on its own
    // workgroups, where a tile's first-layer workgroups are enough to carry its later phases (H / 64 of
    // them the second layer, 4 the last)
    // ... and, round 5, up to 128 tiles (2 048 queries: a rank's share of an 8-GPU batch, the last partial
    // round of a large batch): the 2-7 workgroups a tile then gets take the parts of the later phases in
    // turns (second-layer parts of 128 / 256 columns where a tile has < 8 / < 4 workgroups).  One launch
    // against three (steady state): 513 queries 83 us / 114, 800: 93 / 118, 1 024:
    // 102 / 122, 1 250: 128 / 132, 1 536 - 2 048: 155-156 / 157.  (The first version of this looked SLOWER
    // beyond 816 queries and cost the <= 512-query path 15 us: per-part copies of the argument struct inside
    // the phase loops had put 456 B of it into scratch memory - found through the latency log, now refused by
    // tests/test_host_cpu.py.)  Phase stamps of a tile at 1 250 queries (us): first layer 49, wait 11,
    // activation 4, second layer 21 (6 of them filling LDS), wait 10, last layer 16 (two parts of 64 outputs on
    // the tile's first workgroup), norm 3.
    const bool few_tiles = tiles <= 32 && S * KP >= std::max(std::max(H / 64, 4), (16 * H + 1023) / 1024);
    const bool mid_tiles = tiles > 32 && tiles <= 128 && S * KP >= 2;
    if ((few_tiles || mid_tiles) && n_layers == 2 && enc_fused && H % 64 == 0 && H <= 512 && tiles * S * KP <= n_cu) {
        p.one_launch = true;
        // second-layer parts: 64 columns where the tile has a workgroup for each, else 128 / 256
        p.part2_cols = 64;
        while (p.part2_cols < 256 && S * KP < H / p.part2_cols && H % (2 * p.part2_cols) == 0) p.part2_cols *= 2;
        p.n_parts2 = H / p.part2_cols;
        p.rest_from = 1;
        return p;
    }
    // the second layer over S2 column parts per tile where there are CUs for it (and a second
    // hidden layer exists); the last kernel then starts from its output.  Every part re-reads the
    // tile's partial sums and re-activates them, and a third launch costs its ~10 us: measured
    // (tools/encoder_latency.py, against two launches) 16 queries 106 -> 121 us, 256 queries
    // equal, 625 queries 127 -> 118, 1 250 queries 145 -> 135, 2 048 queries 170 -> 162 us: from 32
    // tiles on.
    // A FEW tiles (up to 8: the latency regime - a handful of queries): one workgroup's chain over the
    // second and the last layer is 12.6 MFLOP of float64 MFMA on ONE CU, 70-90 us whatever the batch.
    // Splitting both layers there too (second: column parts; last: 4 parts of 64 outputs) with a
    // one-wave-per-query kernel to normalise - four short launches instead of two - was MEASURED SLOWER:
    // 133 us against 111 us for 16 queries (round 3; round 2 saw the same with three launches): every
    // dependent launch costs ~10-20 us (dispatch, then 4-6 us before a kernel's first memory access
    // returns), more than the split saves.  What helps is ONE persistent launch (encoder_tile_kernel above).
    int S2 = 1;
    for (int s2 = 2; s2 <= 8 && tiles >= 32 && tiles * s2 <= n_cu && n_layers >= 2; s2 *= 2) {
        const int part = H / s2;
        if (H % s2 == 0 && (part == 64 || part == 128 || part == 256)) S2 = s2;
    }
    p.S2 = S2;
    if (S2 > 1) {
        p.n_parts2 = S2;
        p.part2_cols = H / S2;
        p.rest_from = 1;
    }
    return p;
}

// A batch through the encoder: the leading main_B queries in one launch of encoder_kernel (n_wg32
// workgroups of 32 queries, then workgroups of 16), the split_B queries behind them through the
// small-batch kernels.  Either part may be empty.
struct EncLaunchPlan {
    int64_t main_B = 0;
    int n_wg32 = 0, grid = 0;
    int64_t split_B = 0;
    EncSplitPlan split;
};

inline EncLaunchPlan plan_encoder(int n_cu, int n_slots, int H, int n_layers, bool enc_split, bool enc_fused,
                                  int64_t B, int enc_qtile) {
    EncLaunchPlan p;
    // small batches: the first layer split over column parts and K ranges
    int S, KP;
    choose_encoder_split(n_cu, n_slots, H, (B + 15) / 16, S, KP);
    if (S * KP > 1 && enc_split && split_width_ok(H, S)) {
        p.split_B = B;
        p.split = plan_encoder_split(n_cu, H, n_layers, enc_fused, B, S, KP);
        return p;
    }
    const bool only16 = H > 512;       // (32 queries x H float64 of activations do not fit the LDS)
    // Workgroups take 32 queries and cost the same, one per CU at a time.  When the last round of
    // them would be less than half full, it is run with 16-query workgroups instead (about half
    // the time each): 10 000 queries = 256 x 32 + 113 x 16 instead of 313 x 32.
    const int64_t wg32 = (B + enc_qtile - 1) / enc_qtile;
    const int64_t full_rounds = wg32 / n_cu;
    const int64_t rem = B - full_rounds * n_cu * enc_qtile;      // queries after the full rounds
    // A tail of up to 2 048 queries after full rounds runs as the small-batch kernels (its tiles
    // spread over all CUs: ~0.16 ms for 1 808 queries) instead of a round of 16-query workgroups
    // (0.23 ms whatever its fill): 10 000 queries = 256 x 32 + a split tail of 113 tiles.
    auto main_plus_split_tail = [&](int64_t b_main) -> bool {       // false: not taken
        const int64_t tail = B - b_main;
        choose_encoder_split(n_cu, n_slots, H, (tail + 15) / 16, S, KP);
        if (S * KP <= 1 || !split_width_ok(H, S)) return false;
        // (whole rounds of equal workgroups: the plan of b_main queries is a main launch alone - a tail
        // of its own would be a whole round of tiles, too many to split; host_sanitize.cpp sweeps that)
        p = plan_encoder(n_cu, n_slots, H, n_layers, enc_split, enc_fused, b_main, enc_qtile);
        p.split_B = tail;
        p.split = plan_encoder_split(n_cu, H, n_layers, enc_fused, tail, S, KP);
        return true;
    };
    if (full_rounds > 0 && rem > 0 && rem <= 2048 && enc_split && !only16 && main_plus_split_tail(B - rem)) return p;
    // A batch a little over one round of 16-query workgroups (4 097 .. 5 376 queries on 256 CUs: what a rank
    // of 2 encodes of BASELINE's batch) would fill 60 % of a round of 32-query workgroups and take that
    // round's whole time (0.40 ms): a full round of 16-query workgroups (0.24 ms) + a split tail (<= 0.13 ms)
    const int64_t round16 = (int64_t)16 * n_cu;
    // (the same behind full rounds of 32-query workgroups: 8 192 k + 4 097 .. 5 376 queries)
    if (rem > round16 && rem - round16 <= 1280 && enc_split && !only16 && main_plus_split_tail(B - (rem - round16))) return p;
    p.main_B = B;
    if (only16 || B <= (int64_t)16 * n_cu) {
        // a batch that fits in one round either way: half-size workgroups on twice the CUs
        p.n_wg32 = 0;
        p.grid = (int)((B + 15) / 16);
    } else if (full_rounds > 0 && rem > 0 && rem <= (int64_t)16 * n_cu) {
        p.n_wg32 = (int32_t)(full_rounds * n_cu);
        p.grid = p.n_wg32 + (int)((rem + 15) / 16);
    } else {
        p.n_wg32 = (int32_t)wg32;
        p.grid = (int)wg32;
    }
    return p;
}

// The shift of the softmax statistics and the route of a forward, from the temperatures of a call.
//   SHIFT_CONSTANT     both temperatures <= MAX_TAU_CONSTANT: m = tau * log2(e) (scan_stats_kernel, the
//                      one-pass kernel of small batches): 2^(-2m) stays a normal float32;
//   SHIFT_RUNNING_MAX  either above it: pass 1 is sharp_scan_stats_kernel for BOTH heads (m = the
//                      largest scaled logit), batches of <= 32 queries take the two passes too (the
//                      one-pass kernel keeps the constant shift and its cap), and the in-scan top-k
//                      lists do not exist (top-k comes from the kept logits, or from range_topk_stream).
// Temperatures must be finite, > 0 and <= MAX_TAU_SHARP (tau_geo <= 0: no geographic head); beyond
// that the softmax is an argmax to float32 precision.  (include/range_hip.h: RANGE_MAX_TAU,
// RANGE_MAX_TAU_SHARP are the same numbers; scan_host.h asserts it.)
constexpr float MAX_TAU_CONSTANT = 43.0f;
constexpr float MAX_TAU_SHARP = 1000.0f;
enum ShiftMode { SHIFT_CONSTANT = 0, SHIFT_RUNNING_MAX = 1 };
struct TempRoute {
    bool valid = false;          // false: the temperatures are refused (RANGE_ERR_INVALID)
    ShiftMode shift = SHIFT_CONSTANT;
    bool one_pass = false;       // a forward of B queries takes attend_small_kernel
    bool topk_scan_ok = true;    // the in-scan top-k lists exist for this shift
};

inline bool temperature_ok(float tau, float cap) { return std::isfinite(tau) && tau > 0.f && tau <= cap; }

inline TempRoute plan_temperatures(float tau_sem, float tau_geo, int64_t B, bool small_forward) {
    TempRoute r;
    const bool geo = tau_geo > 0.f;
    if (!temperature_ok(tau_sem, MAX_TAU_SHARP)) return r;
    if (std::isnan(tau_geo) || (geo && !temperature_ok(tau_geo, MAX_TAU_SHARP))) return r;
    r.valid = true;
    const bool sharp = tau_sem > MAX_TAU_CONSTANT || (geo && tau_geo > MAX_TAU_CONSTANT);
    r.shift = sharp ? SHIFT_RUNNING_MAX : SHIFT_CONSTANT;
    r.one_pass = !sharp && small_forward && B > 0 && B <= 32;
    r.topk_scan_ok = !sharp;
    return r;
}

// Pass 1 (scan_stats_kernel) over a chunk of B queries, one workgroup per (bank split, query tile),
// and the streaming top-k over the logits it kept.
struct Pass1Plan {
    int n_qtiles = 0, n_blocks = 0, n_splits = 0;
    int grid = 0;               // n_splits * n_qtiles
    bool merge_by_wave = false; // merge_stats_wave_kernel (one wave per query) instead of merge_stats_kernel
    size_t part_floats = 0;     // statistics (and row maxima) per split: n_splits * B * 4
    int64_t topk_slots = 0;     // top-k from the kept logits: wave slots of 16 queries ...
    int topk_chunks = 0;        // ... x chunks of bank blocks; one candidate list per (chunk, query)
};

// topk_scan: the in-scan candidate lists (contexts that cannot keep logits); force_splits > 0: the
// caller's split count (range_scan_stats_at), clamped to what the bank allows
inline Pass1Plan plan_pass1(int n_cu, int64_t n_rows, int64_t B, bool topk_scan, int force_splits, const PlanConsts& K) {
    Pass1Plan p;
    p.n_blocks = (int32_t)((n_rows + K.blk - 1) / K.blk);
    p.n_qtiles = (int32_t)((B + K.qtile - 1) / K.qtile);
    // small batches are HBM-bound: many splits so that every CU streams a share of the keys
    const bool few = B <= 4 * K.qtile;
    // pass 1 writes 16 B per (query, split): many splits are free
    // in-scan top-k candidates cost 512 B per (query, split) and are merged by one wave per
    // query: keep the split count moderate in that variant
    p.n_splits = choose_splits(p.n_qtiles, p.n_blocks, n_cu, K.p1_wg_per_cu,
                               topk_scan ? (few ? 256 : 16) : (few ? 2048 : 128));
    if (force_splits > 0) p.n_splits = std::max(1, std::min<int>(force_splits, std::max(1, p.n_blocks / 4)));
    p.grid = p.n_splits * p.n_qtiles;
    p.merge_by_wave = p.n_splits > 32;
    p.part_floats = (size_t)p.n_splits * B * 4;
    // enough waves to fill the chip: (B/16 wave slots) x chunks of bank blocks
    p.topk_slots = (B + 15) / 16;
    p.topk_chunks = (int)std::max<int64_t>(1, std::min<int64_t>(
        std::min<int64_t>(64, p.n_blocks / 32 > 0 ? p.n_blocks / 32 : 1),
        ((int64_t)16 * n_cu + p.topk_slots - 1) / p.topk_slots));
    return p;
}

// Statistics from the kept logits (pass1_kept.h: kept_stats_kernel) for B queries at n_pairs temperature
// pairs: pass 1's decomposition - one workgroup per (bank split, query tile) - with up to max_pairs pairs
// per launch; every pair's parts are then merged as pass 1's are.
struct KeptStatsPlan {
    int n_qtiles = 0, n_blocks = 0, n_splits = 0;
    int grid = 0;               // n_splits * n_qtiles
    bool merge_by_wave = false;
    struct Group { int first, count; };
    std::vector<Group> groups;  // the launches: pairs [first, first + count), count <= max_pairs
    size_t part_floats = 0;     // parts of ONE pair: n_splits * B * 4
    size_t ws_floats = 0;       // workspace: the parts of the largest group
};

// the shift of one pair's statistics: the rule of pass 1 (either temperature above 43: the running maximum
// for both heads)
inline ShiftMode kept_pair_shift(float tau_sem, float tau_geo) { return plan_temperatures(tau_sem, tau_geo, 0, false).shift; }

// force_splits: the caller's split count (0: what a scan of B queries chooses) - the rule of
// range_scan_stats_at, clamp included, so that the parts are those of the scan
inline KeptStatsPlan plan_kept_stats(int n_cu, int64_t n_rows, int64_t B, int n_pairs, int force_splits, int max_pairs,
                                     const PlanConsts& K) {
    KeptStatsPlan p;
    const Pass1Plan s = plan_pass1(n_cu, n_rows, B, false, force_splits, K);
    p.n_qtiles = s.n_qtiles;
    p.n_blocks = s.n_blocks;
    p.n_splits = s.n_splits;
    p.grid = s.grid;
    p.merge_by_wave = s.merge_by_wave;
    p.part_floats = s.part_floats;
    for (int first = 0; first < n_pairs; first += max_pairs)
        p.groups.push_back({first, std::min(max_pairs, n_pairs - first)});
    p.ws_floats = p.part_floats * (size_t)std::min(max_pairs, std::max(n_pairs, 0));
    return p;
}

// Pass 2 (attend_kernel / attend_stored_kernel / attend_bf16x3_kernel) over B queries.
struct Pass2Plan {
    int n_qtiles = 0, n_blocks = 0;
    int n_splits = 0;           // split scheme: one workgroup per (bank split, query tile)
    bool streamk = false;
    int sk_cols = 1, sk_groups = 0;   // ScanArgs / SlabMap fields (split scheme: 1, 0)
    int grid = 0;
    size_t slab_floats = 0;     // the slabs the launch writes
};

// allow_streamk: RANGE_P2_STREAMK, and the kernel of this call has the walk (the exact ones); force_splits > 0: the
// caller's split count for the split scheme (a chunk of a forward takes the whole batch's: plan_forward_chunks)
inline Pass2Plan plan_pass2(int n_cu, int64_t n_rows, int64_t B, bool allow_streamk, const PlanConsts& K,
                            int force_splits = 0) {
    Pass2Plan p;
    p.n_blocks = (int32_t)((n_rows + K.blk - 1) / K.blk);
    p.n_qtiles = (int32_t)((B + K.qtile - 1) / K.qtile);
    // pass 2 writes a 4 KB row
    // (a small batch may split pass 2 further, until every CU has a workgroup).  Every extra
    // split of pass 2 writes and re-reads a 4 KB row per query: 8 KB at ~4 TB/s against the
    // query's MFMA time n_rows * 2054 FLOP / 140 TFLOP/s, i.e. 140 / n_rows of the launch - small
    // for the whole bank on one GPU, 1 % per split for a 12 500-row shard.
    p.n_splits = choose_splits(p.n_qtiles, p.n_blocks, n_cu, 1,
                               std::max(32, std::min(512, (n_cu + p.n_qtiles - 1) / p.n_qtiles)),
                               std::max(0.001, 140.0 / (double)n_rows));
    if (force_splits > 0) p.n_splits = std::max(1, std::min<int>(force_splits, std::max(1, p.n_blocks / 4)));
    // Stream-K (scan_common.h: SlabMap): as many workgroups as CUs, each with the same number of
    // (query tile, bank block) units (at least 4: tiny launches take fewer workgroups), one slab per
    // query tile a workgroup touches.  For banks and SHARDS of up to 50 000 rows - measured, 10 000
    // queries, pass 2 + its reduction, against one workgroup per (split, query tile): 12 500 rows (a
    // rank of 8) -5.6 %, 25 000 -3.6 %, 50 000 -2.2 %; at 100 000 rows that scheme's 7.97 rounds of
    // workgroups are 98.5 % full already, the walk gains 0.5-1 % with two 50 000-row columns (and
    // loses 9 % with one: its workgroups re-read the values from HBM then, not from the Infinity
    // Cache) while its longer float32 accumulation chains cost accuracy (|sum of weights - 1| of the
    // worst of 10^5 queries 1.3e-5 instead of 0.5e-5): not taken there.  The exact kernels only;
    // RANGE_P2_STREAMK=0 restores the split scheme for A/B.
    constexpr int P2_STREAMK_ROWS = 50000;
    p.streamk = allow_streamk && n_rows <= P2_STREAMK_ROWS;
    if (p.streamk) {
        // columns of at most 16 384 rows: an accumulation chain (one query tile's blocks of a column)
        // stays within ~2x the 481 blocks of the split scheme on the full bank
        constexpr int P2_COL_ROWS = 16384;
        p.sk_cols = (int32_t)std::max<int64_t>(1, std::min<int64_t>((n_rows + P2_COL_ROWS - 1) / P2_COL_ROWS,
                                                                    std::max(1, p.n_blocks / 4)));
        const int64_t Uc = (int64_t)p.n_qtiles * (p.n_blocks / p.sk_cols);     // (units of the shortest column)
        p.sk_groups = (int32_t)std::max<int64_t>(1, std::min<int64_t>(n_cu, Uc / 4));
        p.slab_floats = (size_t)p.sk_cols * (p.sk_groups + p.n_qtiles) * K.qtile * K.val_dim;
    } else {
        p.slab_floats = (size_t)p.n_splits * B * K.val_dim;
    }
    p.grid = p.streamk ? p.sk_groups : p.n_splits * p.n_qtiles;
    return p;
}

// range_forward in chunks of query tiles (forward_host.h): pass 1 of chunk i + 1 runs on the CUs that pass 2 of
// chunk i occupies (pass1_beside.h).  Every chunk takes the WHOLE batch's split counts of both passes (p1, p2: the
// plans of all B queries): split boundaries depend on the bank's blocks and the split count only, the merge and
// finalize orders on the split count only, so a chunked forward gives the bits of the single launches.
struct FwdChunkPlan {
    std::vector<int> tiles;             // query tiles of every chunk, in order; empty: no chunking
    int p1_splits = 0, p2_splits = 0;
};

// overlap: RANGE_FWD_OVERLAP - 0 never, n > 0 chunks of n query tiles (tests), < 0 the rule:
//   each chunk is a whole number of pass 2's rounds of n_cu workgroups, filled to FWD_CHUNK_FILL_PCT at least, and the
//   chunks' rounds sum to the single launch's (no round is added);
//   as many chunks as a near-equal division of the rounds allows (parts that differ by at most one round, the
//   shorter ones first); the tiles a chunk could still take are missing in the first chunks: the smallest chunk
//   comes first, its pass 1 is the exposed one.
//   The benchmark - 256 CUs, 157 tiles x 13 splits = 2 041 workgroups in 8 rounds: 39 + 59 + 59 tiles
//   (507, 767, 767 workgroups in 2, 3, 3 rounds).
// No chunking for the stream-K walk of pass 2 (its workgroups are already one even round) and below two chunks.
constexpr int FWD_CHUNK_FILL_PCT = 98;
inline FwdChunkPlan plan_forward_chunks(int n_cu, const Pass1Plan& p1, const Pass2Plan& p2, int overlap) {
    FwdChunkPlan p;
    p.p1_splits = p1.n_splits;
    p.p2_splits = p2.n_splits;
    const int T = p2.n_qtiles, ns = p2.n_splits;
    if (overlap == 0 || p2.streamk || T < 2 || ns < 1 || n_cu < 1) return p;
    if (overlap > 0) {
        for (int t0 = 0; t0 < T && overlap < T; t0 += overlap) p.tiles.push_back(std::min(overlap, T - t0));
        return p;
    }
    const int64_t R = ((int64_t)T * ns + n_cu - 1) / n_cu;
    for (int64_t C = std::min<int64_t>(R, T); C >= 2; --C) {
        std::vector<int> lo((size_t)C), hi((size_t)C);
        int64_t sum_lo = 0, sum_hi = 0;
        bool ok = true;
        for (int64_t i = 0; i < C && ok; ++i) {
            const int64_t r = R / C + (i >= C - R % C ? 1 : 0);
            // tiles whose workgroups make exactly r rounds: at most r n_cu of them, more than (r - 1) n_cu, and
            // FWD_CHUNK_FILL_PCT of r n_cu
            const int64_t most = r * n_cu / ns;
            const int64_t fill = (FWD_CHUNK_FILL_PCT * r * n_cu + 100 * (int64_t)ns - 1) / (100 * (int64_t)ns);
            const int64_t least = std::max<int64_t>(std::max<int64_t>(fill, (r - 1) * n_cu / ns + 1), 1);
            ok = least <= most;
            lo[(size_t)i] = (int)least;
            hi[(size_t)i] = (int)most;
            sum_lo += least;
            sum_hi += most;
        }
        if (!ok || sum_lo > T || sum_hi < T) continue;
        p.tiles = hi;
        int64_t excess = sum_hi - T;
        for (size_t i = 0; i < p.tiles.size() && excess > 0; ++i) {
            const int64_t d = std::min<int64_t>(excess, hi[i] - lo[i]);
            p.tiles[i] -= (int)d;
            excess -= d;
        }
        return p;
    }
    return p;
}

// range_topk_stream: the batch-scale GEMM route (topk_gemm.h) or the persistent streaming scan
// (topk_stream.h).
struct TopkPlan {
    int n_groups = 0, n_blocks = 0;   // query groups of 16, bank blocks
    bool gemm = false;
    // streaming scan
    int G = 1;                  // query groups sharing one pass over the keys
    int n_wg = 0;               // persistent grid
    bool fused = false;         // the merge as the tail of the stream kernel
    size_t cand_keys = 0, cand_dmax = 0;   // candidate lists / their bounds: one per (query, workgroup)
    // GEMM route
    int key_e2 = 0;             // key_norm_max < 2^key_e2: the fp16 copy of the keys is scaled by 2^(14 - key_e2)
    int n_qblocks = 0, n_splits = 0, grid = 0;
    int tile_stride = 1;        // pass A looks at every tile_stride-th tile
};

inline TopkPlan plan_topk(int n_cu, int64_t n_rows, int64_t B, float key_norm_max, bool topk_gemm, bool bf16,
                          bool topks_fused, bool force_exact, int tg_sample, const PlanConsts& K) {
    TopkPlan p;
    p.n_groups = (int)((B + 15) / 16);
    p.n_blocks = (int)((n_rows + K.blk - 1) / K.blk);
    // persistent grid: one workgroup per CU (its key tiles fill the LDS), 4 waves each streaming
    // its own tiles; one candidate list of 8 per (query, workgroup).  Query groups sharing one pass
    // over the keys: 2 groups (32 queries) are still at the ridge (16 FLOP per key byte) and take
    // the time of 1.3.
    constexpr int NWV = 4;
    // (the bf16 prefilter with FOUR groups per pass was measured too: one pass for 64 queries takes
    // 27.0 us against 28.7 us for two passes of two groups - the list work per group, not the
    // stream, is what a pass costs by then - and needs 370 registers; not kept)
    p.G = p.n_groups <= 1 ? 1 : 2;     // query groups (of 16) sharing one pass over the keys
    p.n_wg = std::max(1, std::min(std::min(n_cu, 256), (p.n_blocks + NWV - 1) / NWV));
    // the merge runs as the tail of the stream kernel while every query finds a workgroup of its own
    p.fused = topks_fused && B <= p.n_wg;
    p.cand_keys = (size_t)p.n_groups * 16 * p.n_wg * K.topks_wl;
    p.cand_dmax = (size_t)p.n_groups * 16 * p.n_wg;
    // (the candidate lists of a call are addressed by 32-bit byte offsets: B x lists x 256 B < 4 GB - the
    // Python layer calls in chunks of 16 384 queries = 1 GB at most)
    // (a bank whose largest key norm is so far from 1 that no power of two brings it into fp16's range - or
    // that is all zeros - keeps the streaming scan)
    (void)std::frexp((double)key_norm_max, &p.key_e2);                  // key_norm_max < 2^e2
    const bool tg_bank_ok = key_norm_max > 0.f && std::isfinite(key_norm_max) && std::abs(14 - p.key_e2) <= 100;
    p.gemm = topk_gemm && bf16 && B > 256 && p.n_blocks >= 64 && !force_exact && B <= 60000 && tg_bank_ok;
    if (p.gemm) {
        // batches beyond the one-launch regime: GEMM-shaped, list-free (topk_gemm.h): group maxima ->
        // per-query threshold -> candidates -> float32 re-rank.  Two workgroups per CU; the splits fill
        // one round of them (at least 4: 32 row groups for the threshold; at least 8 tiles each).
        p.n_qblocks = (int32_t)((B + K.tg_qblock - 1) / K.tg_qblock);
        p.n_splits = std::max(4, std::min(std::min(K.tg_wg_per_cu * n_cu / p.n_qblocks, p.n_blocks / 8), 64));
        p.grid = p.n_qblocks * p.n_splits;
        p.tile_stride = std::max(1, std::min(tg_sample, p.n_blocks / p.n_splits / 4));
    }
    return p;
}

// range_forward of up to 32 queries: the whole retrieval in one pass over the bank (attend_small.h),
// every workgroup its share of the bank blocks and all the queries (nq tiles of 16).
struct SmallPlan {
    int n_blocks = 0, n_wg = 0;
    int nq = 1, qcap = 16;              // query tiles of a workgroup, queries they hold
    size_t o_floats = 0, z_floats = 0;  // per-workgroup partial products (both heads) / weight sums
};

inline SmallPlan plan_forward_small(int n_cu, int64_t n_rows, int64_t B, const PlanConsts& K) {
    SmallPlan p;
    p.n_blocks = (int)((n_rows + K.blk - 1) / K.blk);
    p.n_wg = std::max(1, std::min(n_cu, p.n_blocks));
    p.nq = B > 16 ? 2 : 1;
    p.qcap = 16 * p.nq;            // query tiles of a workgroup
    p.o_floats = (size_t)p.n_wg * 2 * p.qcap * K.val_dim;
    p.z_floats = (size_t)p.n_wg * p.qcap * 2;
    return p;
}

// The training-free positional encoders (posenc_kernel.h; range_posenc_features).  Kinds, and the
// outputs one frequency contributes to a row: Theory 6 (sin, cos of three angles), grid 4 (sin, cos of
// lon and of lat), the sphere kinds 2T - T terms, each written twice.
enum { PE_THEORY = 0, PE_GRID = 1, PE_SPHEREC = 2, PE_SPHERECPLUS = 3, PE_SPHEREM = 4, PE_SPHEREMPLUS = 5,
       PE_KINDS = 6 };
constexpr int POSENC_BLOCK = 256;                  // work items (location, frequency) of a tile = threads of a workgroup
constexpr int POSENC_MAX_F = 64;
constexpr int64_t POSENC_MAX_GRID = 1 << 20;       // workgroups of a launch; more tiles are walked grid-stride
RANGE_HD constexpr int posenc_per_freq(int kind) {
    return kind == PE_THEORY ? 6 : kind == PE_GRID ? 4 : kind == PE_SPHEREC ? 6 : kind == PE_SPHERECPLUS ? 12
         : kind == PE_SPHEREM ? 10 : kind == PE_SPHEREMPLUS ? 16 : 0;
}

struct PosencPlan {
    bool valid = false;
    int per_freq = 0, width = 0;        // outputs per frequency; row width = F * per_freq
    int64_t items = 0, n_tiles = 0;     // B * F work items in tiles of POSENC_BLOCK
    unsigned grid = 0;
    int block = POSENC_BLOCK;
    bool staged = false;                // the tile's outputs go through LDS and are written out linearly (all kinds but grid)
    int locs_per_tile = 0;              // spherem / spheremplus: most locations a tile touches
    size_t lds_bytes = 0;
    // tiles workgroup `blk` walks: blk, blk + grid, ... below n_tiles
    int64_t tiles_of(int64_t blk) const { return blk < n_tiles ? (n_tiles - blk + grid - 1) / grid : 0; }
};

// Invalid: unknown kind, F outside 1 .. POSENC_MAX_F, B < 1, or an output of more than 2^62 bytes.
inline PosencPlan posenc_plan(int kind, int F, int64_t B) {
    PosencPlan p;
    p.per_freq = posenc_per_freq(kind);
    if (!p.per_freq || F < 1 || F > POSENC_MAX_F || B < 1) return p;
    p.width = F * p.per_freq;
    if (B > (INT64_C(1) << 59) / p.width) return p;
    p.items = B * F;
    p.n_tiles = (p.items + POSENC_BLOCK - 1) / POSENC_BLOCK;
    p.grid = (unsigned)std::min(p.n_tiles, POSENC_MAX_GRID);
    p.staged = kind != PE_GRID;
    if (kind == PE_SPHEREM || kind == PE_SPHEREMPLUS)
        p.locs_per_tile = (F - 1 + POSENC_BLOCK - 1) / F + 1;     // a tile may start at frequency F - 1 of a location
    p.lds_bytes = ((p.staged ? (size_t)POSENC_BLOCK * p.per_freq : 0) + (size_t)3 * p.locs_per_tile) * sizeof(double);
    p.valid = true;
    return p;
}

// The CSP location encoders (csp_kernel.h; range_set_csp / range_csp_encode): 'gridcell' or 'theory'
// features of F frequencies, then n_layers float32 linear layers - every one followed by the activation,
// the hidden ones (all but the last) also by the skip connection (where input and output width agree)
// and torch's LayerNorm.  A workgroup of CSP_BLOCK threads takes a tile of 64 locations (32 when a width
// is beyond 512: the layer's whole output tile lives in the four waves' accumulators, 128 registers a
// lane) whose activations stay in ONE LDS image of `ld` floats a row; `ld` is odd, so the 32 rows an MFMA
// A operand reads fall into 32 banks.  Weights are packed per layer in the order the kernel reads them
// (csp_pack_weights): K padded to CSP_KGROUP, N to CSP_NTILE, with zeros.
enum { CSP_ACT_SIGMOID = 0, CSP_ACT_RELU = 1, CSP_ACT_LEAKYRELU = 2, CSP_ACT_TANH = 3, CSP_ACT_GELU = 4, CSP_ACTS = 5 };
constexpr int CSP_BLOCK = 256;
constexpr int CSP_MAX_F = 64, CSP_MAX_WIDTH = 1024, CSP_MAX_LAYERS = 9;   // <= 8 hidden layers and the output layer
constexpr int CSP_KGROUP = 8;             // k of one 16-byte weight fragment: four 32x32x2 steps
constexpr int CSP_NTILE = 32;             // output columns of one MFMA tile
constexpr int CSP_ACC_TILES = 8;          // 32x32 accumulator tiles of a wave: m_tiles * (n tiles of the wave)
constexpr int64_t CSP_MAX_GRID = 2048;    // workgroups of a launch (one fits a CU); more tiles are walked grid-stride

// The grid of a launch over `items`: at most CSP_MAX_GRID workgroups, or the smaller cap `max_grid` (0: none).
inline unsigned csp_grid_cap(int64_t items, int64_t max_grid) {
    return (unsigned)std::min(items, max_grid ? std::min(max_grid, CSP_MAX_GRID) : CSP_MAX_GRID);
}

struct CspLayerPlan {
    int in = 0, out = 0;                 // true widths
    int k_groups = 0, n_tiles = 0;       // ceil(in / CSP_KGROUP), ceil(out / CSP_NTILE)
    bool skip = false, layn = false;
    size_t w_off = 0, b_off = 0, g_off = 0, be_off = 0;   // floats into the packed parameters (g/be: layn only)
    int k_pad() const { return k_groups * CSP_KGROUP; }
    int n_pad() const { return n_tiles * CSP_NTILE; }
};

struct CspPlan {
    bool valid = false;
    const char* why = "";                // what is outside the envelope
    int in0 = 0, out_width = 0, n_layers = 0;
    CspLayerPlan layer[CSP_MAX_LAYERS];
    int tile_rows = 0, m_tiles = 0, ld = 0;
    size_t lds_bytes = 0, packed_floats = 0;
    int64_t n_tiles = 0;
    unsigned grid = 0;
    int block = CSP_BLOCK;
    int64_t tiles_of(int64_t blk) const { return blk < n_tiles ? (n_tiles - blk + grid - 1) / grid : 0; }
};

// kind: PE_GRID or PE_THEORY.  widths[i]: output width of layer i (n_layers >= 1; the last is num_filts).
// max_grid: a smaller cap on the grid than CSP_MAX_GRID (0: none) - for tests of the grid-stride walk.
inline CspPlan csp_plan(int kind, int F, int n_layers, const int* widths, bool skip, bool use_layn, int64_t B,
                        int64_t max_grid = 0) {
    CspPlan p;
    if (kind != PE_GRID && kind != PE_THEORY) { p.why = "spa_enc kind (gridcell or theory)"; return p; }
    if (F < 1 || F > CSP_MAX_F) { p.why = "frequency_num outside 1 .. 64"; return p; }
    if (n_layers < 1 || n_layers > CSP_MAX_LAYERS || !widths) { p.why = "more than 8 hidden layers"; return p; }
    if (B < 1 || B > (INT64_C(1) << 48) || max_grid < 0) { p.why = "batch size"; return p; }
    p.in0 = posenc_per_freq(kind) * F;
    p.n_layers = n_layers;
    int widest = p.in0, in = p.in0;
    size_t off = 0;
    for (int i = 0; i < n_layers; ++i) {
        const int out = widths[i];
        if (out < 1 || out > CSP_MAX_WIDTH) { p.why = "layer width outside 1 .. 1024"; return p; }
        CspLayerPlan& l = p.layer[i];
        l.in = in;
        l.out = out;
        l.k_groups = (in + CSP_KGROUP - 1) / CSP_KGROUP;
        l.n_tiles = (out + CSP_NTILE - 1) / CSP_NTILE;
        const bool hidden = i + 1 < n_layers;
        l.skip = hidden && skip && in == out;
        l.layn = hidden && use_layn;
        l.w_off = off;
        off += (size_t)l.k_pad() * l.n_pad();
        l.b_off = off;
        off += l.n_pad();
        if (l.layn) { l.g_off = off; l.be_off = off + l.n_pad(); off += 2 * (size_t)l.n_pad(); }
        widest = std::max(widest, out);
        in = out;
    }
    p.out_width = in;
    p.packed_floats = off;
    p.m_tiles = widest <= 512 ? 2 : 1;
    p.tile_rows = 32 * p.m_tiles;
    // a row holds any layer's input padded to CSP_KGROUP and any output padded to CSP_NTILE; odd
    p.ld = (widest + CSP_NTILE - 1) / CSP_NTILE * CSP_NTILE + 1;
    p.lds_bytes = (size_t)p.tile_rows * p.ld * sizeof(float);
    p.n_tiles = (B + p.tile_rows - 1) / p.tile_rows;
    p.grid = csp_grid_cap(p.n_tiles, max_grid);
    p.valid = true;
    return p;
}

// where W[n][k] of a layer goes in its packed weights: (n tile, k group, lane, step) with lane = 32 * (k & 1)
// + n % 32 and step = (k % 8) / 2 - lane `l` of a wave reads the four floats of its k group at once and feeds
// step s of them to the MFMA as B[k = l >> 5][n = l & 31]
inline size_t csp_packed_index(const CspLayerPlan& l, int n, int k) {
    const int nt = n / CSP_NTILE, kg = k / CSP_KGROUP, kk = k % CSP_KGROUP;
    const int lane = 32 * (kk & 1) + n % CSP_NTILE;
    return (((size_t)nt * l.k_groups + kg) * 64 + lane) * 4 + kk / 2;
}

// one layer's parameters into `dst` (p.packed_floats floats, zeroed by the caller): weight (out, in) row-major,
// bias (out), and gamma / beta (out) where the layer has a LayerNorm
inline void csp_pack_layer(const CspPlan& p, int i, const float* weight, const float* bias, const float* gamma,
                           const float* beta, float* dst) {
    const CspLayerPlan& l = p.layer[i];
    for (int n = 0; n < l.out; ++n) {
        for (int k = 0; k < l.in; ++k) dst[l.w_off + csp_packed_index(l, n, k)] = weight[(size_t)n * l.in + k];
        dst[l.b_off + n] = bias[n];
        if (l.layn) { dst[l.g_off + n] = gamma[n]; dst[l.be_off + n] = beta[n]; }
    }
}

// The composed calls (range_csp_predict, range_csp_predict_rank) encode a chunk of locations into a workspace and run
// the head on it: rows of a chunk for embeddings `width` wide - at most 2^16, at most 64 MiB of float32, whole 64-row tiles.
inline int64_t csp_predict_chunk(int width) { return std::min<int64_t>(INT64_C(1) << 16, (INT64_C(1) << 24) / width / 64 * 64); }

// The CSP class head (csp_head_kernel.h; range_set_csp_head / range_csp_head): sigmoid(X W^T) of (B, num_filts)
// embeddings and the (num_classes, num_filts) class_emb, bias-free - all classes, or the M classes an id array
// names.  A workgroup of CSP_BLOCK threads holds a tile of 64 rows of X (32 when num_filts > 512: the LDS rule
// of the layers) in LDS, row stride `ld` odd, and finishes `cols_per_pass` columns of it per pass: every wave
// CSP_HEAD_ACC_TILES / m_tiles column tiles, dealt round-robin.  (Half the layers' CSP_ACC_TILES: 64 accumulator
// registers leave room for two workgroups a CU, so that one's loads, sigmoids and stores run under the other's
// MFMAs - the head has no second layer to keep a tile resident for.)  A work item is a row tile with
// `chunks_per_item` consecutive chunks of columns (the X tile is loaded once per item): all chunks for SUM, else
// the largest of 8, 4, 2, 1 that still leaves CSP_MAX_GRID items.  item = row tile * groups + group.  Items are
// walked grid-stride under the grid cap.  class_emb is packed like a layer's weight (csp_packed_index).
enum { CSP_HEAD_PROBS = 0, CSP_HEAD_LOGITS = 1, CSP_HEAD_SUM = 2, CSP_HEAD_MODES = 3 };
constexpr int CSP_HEAD_ACC_TILES = 4;                 // 32x32 accumulator tiles of a wave
constexpr int CSP_MAX_CLASSES = 32768;
constexpr int CSP_HEAD_MAX_M = 1 << 24;               // ids of one call (an id may repeat)
constexpr int64_t CSP_HEAD_MAX_B = INT64_C(1) << 40;

struct CspHeadPlan {
    bool valid = false;
    const char* why = "";
    int num_filts = 0, num_classes = 0, M = 0, mode = 0;
    int tile_rows = 0, m_tiles = 0, ld = 0;
    int k_groups = 0, n_tiles = 0;       // of the packed class_emb: ceil(num_filts / 8), ceil(num_classes / 32)
    int wave_tiles = 0;                  // column tiles a wave holds: CSP_HEAD_ACC_TILES / m_tiles
    int cols_per_pass = 0;               // 4 waves * wave_tiles * 32
    int col_tiles = 0, n_chunks = 0;     // ceil(M / 32), ceil(M / cols_per_pass)
    int chunks_per_item = 0, groups = 0; // groups = ceil(n_chunks / chunks_per_item) items a row tile
    int64_t row_tiles = 0, n_items = 0;
    size_t lds_bytes = 0, packed_floats = 0;
    unsigned grid = 0;
    int block = CSP_BLOCK;
    // the packed class_emb as a layer of csp_packed_index
    CspLayerPlan layer() const {
        CspLayerPlan l;
        l.in = num_filts; l.out = num_classes; l.k_groups = k_groups; l.n_tiles = n_tiles;
        return l;
    }
    int64_t items_of(int64_t blk) const { return blk < n_items ? (n_items - blk + grid - 1) / grid : 0; }
    // item -> its row tile and its chunks [chunk0, chunk1)
    void item(int64_t it, int64_t& row_tile, int& chunk0, int& chunk1) const {
        row_tile = it / groups;
        chunk0 = (int)(it - row_tile * groups) * chunks_per_item;
        chunk1 = std::min(chunk0 + chunks_per_item, n_chunks);
    }
    // the column tiles wave `w` (0 .. 3) computes in chunk `ch`: the first, and how many (stride 4)
    int wave_first_tile(int ch, int w) const { return ch * 4 * wave_tiles + w; }
    int wave_n_tiles(int ch, int w) const {
        const int t0 = wave_first_tile(ch, w);
        return col_tiles > t0 ? std::min(wave_tiles, (col_tiles - t0 + 3) / 4) : 0;
    }
};

// M: columns of the call (num_classes without an id array).  max_grid: a smaller cap than CSP_MAX_GRID (0: none).
inline CspHeadPlan csp_head_plan(int num_filts, int num_classes, int64_t M, int64_t B, int mode, int64_t max_grid = 0) {
    CspHeadPlan p;
    if (num_filts < 1 || num_filts > CSP_MAX_WIDTH) { p.why = "num_filts outside 1 .. 1024"; return p; }
    if (num_classes < 1 || num_classes > CSP_MAX_CLASSES) { p.why = "num_classes outside 1 .. 32768"; return p; }
    if (mode < 0 || mode >= CSP_HEAD_MODES) { p.why = "mode (PROBS, LOGITS or SUM)"; return p; }
    if (M < 1 || M > CSP_HEAD_MAX_M) { p.why = "M outside 1 .. 2^24"; return p; }
    if (mode == CSP_HEAD_SUM && M != num_classes) { p.why = "SUM runs over all classes"; return p; }
    if (B < 1 || B > CSP_HEAD_MAX_B || max_grid < 0) { p.why = "batch size"; return p; }
    p.num_filts = num_filts; p.num_classes = num_classes; p.M = (int)M; p.mode = mode;
    p.m_tiles = num_filts <= 512 ? 2 : 1;
    p.tile_rows = 32 * p.m_tiles;
    p.k_groups = (num_filts + CSP_KGROUP - 1) / CSP_KGROUP;
    p.n_tiles = (num_classes + CSP_NTILE - 1) / CSP_NTILE;
    p.ld = p.k_groups * CSP_KGROUP + 1;                  // odd
    p.wave_tiles = CSP_HEAD_ACC_TILES / p.m_tiles;
    p.cols_per_pass = 4 * p.wave_tiles * CSP_NTILE;
    p.col_tiles = (p.M + CSP_NTILE - 1) / CSP_NTILE;
    p.n_chunks = (p.M + p.cols_per_pass - 1) / p.cols_per_pass;
    p.row_tiles = (B + p.tile_rows - 1) / p.tile_rows;
    p.chunks_per_item = 1;
    if (mode == CSP_HEAD_SUM) p.chunks_per_item = p.n_chunks;
    else
        for (int g = 8; g > 1; g /= 2)
            if (p.row_tiles * ((p.n_chunks + g - 1) / g) >= CSP_MAX_GRID) { p.chunks_per_item = g; break; }
    p.groups = (p.n_chunks + p.chunks_per_item - 1) / p.chunks_per_item;
    p.n_items = p.row_tiles * p.groups;
    // X tile, and (SUM) the four waves' partial row sums
    p.lds_bytes = ((size_t)p.tile_rows * p.ld + (size_t)4 * p.tile_rows) * sizeof(float);
    p.packed_floats = (size_t)p.n_tiles * CSP_NTILE * p.k_groups * CSP_KGROUP;
    p.grid = csp_grid_cap(p.n_items, max_grid);
    p.valid = true;
    return p;
}

// class_emb (num_classes, num_filts) row-major into `dst` (p.packed_floats floats, zeroed by the caller)
inline void csp_pack_head(const CspHeadPlan& p, const float* class_emb, float* dst) {
    const CspLayerPlan l = p.layer();
    for (int n = 0; n < p.num_classes; ++n)
        for (int k = 0; k < p.num_filts; ++k) dst[csp_packed_index(l, n, k)] = class_emb[(size_t)n * p.num_filts + k];
}

// The evaluation behind the class head (csp_rank_kernel.h; range_csp_rank): per row the true class's rank counts
// and the arg-max of s_c = p_c * img[b, c] over ALL classes, the head's tile and chunks (csp_head_plan in PROBS
// mode, M = num_classes) with the image predictions read where the head would store.  A work item is a row tile
// with one of `col_parts` consecutive, balanced shares of the chunks: item = row tile * col_parts + part.  The
// row tiles alone fill the chip from CSP_RANK_TARGET_WG on (256 CUs x 2 workgroups); below that col_parts is the
// smallest number of parts that reaches it, at most one part a chunk.  With more than one part the partial
// (greater, tied_after, best score, best index) take col_parts * B * 20 bytes of workspace and a merge launch
// follows.  Without embeddings (has_head = false: the reference's 'no_prior') no X tile is held and the tile is
// 64 rows.  LDS behind the X tile, per row: four waves' {s_t, best} (16 bytes each), s_t (8), four waves' best
// index, greater and tied counts (4 bytes each), the label (4).
enum { CSP_IMG_NONE = 0, CSP_IMG_F32 = 1, CSP_IMG_F64 = 2, CSP_IMG_KINDS = 3 };
constexpr int64_t CSP_RANK_TARGET_WG = 512;
constexpr size_t CSP_RANK_ROW_STATE = 4 * 16 + 8 + 3 * 4 * 4 + 4;     // bytes of LDS a row beside the X tile
constexpr size_t CSP_RANK_WS_ROW = 8 + 3 * 4;                         // bytes of workspace a row and part

struct CspRankPlan {
    bool valid = false;
    const char* why = "";
    int num_filts = 0, num_classes = 0, img_kind = 0;
    bool has_head = false;
    int tile_rows = 0, m_tiles = 0, ld = 0, k_groups = 0;
    int wave_tiles = 0, cols_per_pass = 0, col_tiles = 0;
    int n_chunks = 0;                    // ceil(num_classes / cols_per_pass)
    int col_parts = 0;
    int64_t row_tiles = 0, n_items = 0;
    size_t lds_bytes = 0, ws_bytes = 0;  // ws_bytes: 0 with one part
    unsigned grid = 0, merge_grid = 0;   // merge_grid: 0 with one part
    int block = CSP_BLOCK;
    int64_t items_of(int64_t blk) const { return blk < n_items ? (n_items - blk + grid - 1) / grid : 0; }
    // item -> its row tile, its part and the part's chunks [chunk0, chunk1)
    void item(int64_t it, int64_t& row_tile, int& part, int& chunk0, int& chunk1) const {
        row_tile = it / col_parts;
        part = (int)(it - row_tile * col_parts);
        chunk0 = (int)((int64_t)part * n_chunks / col_parts);
        chunk1 = (int)((int64_t)(part + 1) * n_chunks / col_parts);
    }
    // the column tiles wave `w` (0 .. 3) sweeps in chunk `ch`: the first, and how many (stride 4) - the head's
    int wave_first_tile(int ch, int w) const { return ch * 4 * wave_tiles + w; }
    int wave_n_tiles(int ch, int w) const {
        const int t0 = wave_first_tile(ch, w);
        return col_tiles > t0 ? std::min(wave_tiles, (col_tiles - t0 + 3) / 4) : 0;
    }
};

// img_kind: CSP_IMG_*.  has_head: embeddings are given.  max_grid: a smaller cap than CSP_MAX_GRID (0: none).
// col_parts: 0 the plan's choice, n > 0 exactly n parts.
inline CspRankPlan csp_rank_plan(int num_filts, int num_classes, int64_t B, int img_kind, bool has_head,
                                 int64_t max_grid = 0, int col_parts = 0) {
    CspRankPlan p;
    if (img_kind < 0 || img_kind >= CSP_IMG_KINDS) { p.why = "img_kind (NONE, F32 or F64)"; return p; }
    if (!has_head && img_kind == CSP_IMG_NONE) { p.why = "neither embeddings nor image predictions"; return p; }
    if (col_parts < 0) { p.why = "col_parts below 0"; return p; }
    const CspHeadPlan h = csp_head_plan(num_filts, num_classes, num_classes, B, CSP_HEAD_PROBS, max_grid);
    if (!h.valid) { p.why = h.why; return p; }
    p.num_filts = num_filts; p.num_classes = num_classes; p.img_kind = img_kind; p.has_head = has_head;
    p.m_tiles = has_head ? h.m_tiles : 2;
    p.tile_rows = 32 * p.m_tiles;
    p.k_groups = h.k_groups;
    p.ld = h.ld;
    p.wave_tiles = CSP_HEAD_ACC_TILES / p.m_tiles;
    p.cols_per_pass = 4 * p.wave_tiles * CSP_NTILE;
    p.col_tiles = h.col_tiles;
    p.n_chunks = (num_classes + p.cols_per_pass - 1) / p.cols_per_pass;
    if (col_parts > p.n_chunks) { p.why = "col_parts above the number of chunks"; return p; }
    p.row_tiles = (B + p.tile_rows - 1) / p.tile_rows;
    p.col_parts = col_parts ? col_parts
                            : (int)std::min<int64_t>(p.n_chunks, (CSP_RANK_TARGET_WG + p.row_tiles - 1) / p.row_tiles);
    p.n_items = p.row_tiles * p.col_parts;
    p.lds_bytes = (has_head ? (size_t)p.tile_rows * p.ld * sizeof(float) : 0) + (size_t)p.tile_rows * CSP_RANK_ROW_STATE;
    p.grid = csp_grid_cap(p.n_items, max_grid);
    if (p.col_parts > 1) {
        p.ws_bytes = (size_t)p.col_parts * (size_t)B * CSP_RANK_WS_ROW;
        p.merge_grid = (unsigned)std::min<int64_t>((B + CSP_BLOCK - 1) / CSP_BLOCK, CSP_MAX_GRID);
    }
    p.valid = true;
    return p;
}

// The nearest-support scan of the checkerboard task (checker_kernel.h; range_nearest_support): one thread per
// query, workgroups of CHECKER_BLOCK queries (grid x, walked grid-stride), support tiles of CHECKER_TILE points
// in LDS (lon, lat, cos lat: 3 doubles a point), the tiles dealt round-robin to `chunks` workgroups per query
// block (grid y).  Q alone fills the chip only from CHECKER_TARGET_WG query blocks on (2048 = 256 CUs x 8
// workgroups of 4 waves, the CU's 32 waves): below that the support is split so that query blocks x chunks
// reaches it, every chunk keeping at least one tile, at most CHECKER_MAX_CHUNKS.  With more than one chunk
// the partial (a, index) pairs take chunks * Q * 16 bytes of workspace and a merge launch follows.
constexpr int CHECKER_BLOCK = 256;
constexpr int CHECKER_TILE = 256;
constexpr int CHECKER_MAX_CHUNKS = 64;
constexpr int64_t CHECKER_TARGET_WG = 2048;
constexpr int64_t CHECKER_MAX_GRID = 1 << 20;      // query blocks of a launch; more are walked grid-stride
constexpr int64_t CHECKER_MAX_POINTS = INT64_C(1) << 40;

struct CheckerPlan {
    bool valid = false;
    int tile = CHECKER_TILE, block = CHECKER_BLOCK;
    int64_t q_blocks = 0, s_tiles = 0;
    unsigned grid_x = 0;                // workgroups over the query blocks
    int chunks = 0;                     // grid y
    unsigned merge_grid = 0;            // chunks > 1: workgroups of the merge launch
    size_t lds_bytes = 0;
    size_t ws_pairs = 0, ws_bytes = 0;  // chunks > 1: chunks * Q partial pairs, a double and an int64 each
    // query blocks workgroup x walks (x, x + grid_x, ...); tiles chunk y walks (y, y + chunks, ...)
    int64_t blocks_of(int64_t x) const { return x < q_blocks ? (q_blocks - x + grid_x - 1) / grid_x : 0; }
    int64_t tiles_of(int64_t y) const { return y < s_tiles ? (s_tiles - y + chunks - 1) / chunks : 0; }
};

// max_chunks: 0 the plan's choice, n > 0 at most n chunks (tests of the split; never more than the tiles).
// Invalid: Q or S < 1 or beyond 2^40, exclude_self with Q != S or S < 2, a negative max_chunks.
inline CheckerPlan checker_plan(int64_t Q, int64_t S, bool exclude_self, int max_chunks) {
    CheckerPlan p;
    if (Q < 1 || S < 1 || Q > CHECKER_MAX_POINTS || S > CHECKER_MAX_POINTS || max_chunks < 0) return p;
    if (exclude_self && (Q != S || S < 2)) return p;
    p.q_blocks = (Q + CHECKER_BLOCK - 1) / CHECKER_BLOCK;
    p.s_tiles = (S + CHECKER_TILE - 1) / CHECKER_TILE;
    p.grid_x = (unsigned)std::min(p.q_blocks, CHECKER_MAX_GRID);
    const int64_t want = max_chunks > 0 ? (int64_t)max_chunks : (CHECKER_TARGET_WG + p.q_blocks - 1) / p.q_blocks;
    p.chunks = (int)std::min(std::min(want, p.s_tiles), (int64_t)CHECKER_MAX_CHUNKS);
    p.lds_bytes = (size_t)3 * CHECKER_TILE * sizeof(double);
    if (p.chunks > 1) {
        p.ws_pairs = (size_t)p.chunks * (size_t)Q;
        p.ws_bytes = p.ws_pairs * 16;
        p.merge_grid = (unsigned)std::min(p.q_blocks, CHECKER_MAX_GRID);
    }
    p.valid = true;
    return p;
}

// The embedding map (map_kernels.h; include/range_map.h).  Three row walks over n rows:
//   * projection: a workgroup of MAP_BLOCK threads takes MAP_PROJ_ROWS rows a trip (MAP_PROJ_WAVE_ROWS per
//     wave), the grid is capped at MAP_MAX_GRID workgroups and walks the row groups grid-stride;
//   * ICA step: the rows are cut into slabs of `chunk` = MAP_BLOCK * ipt rows, a cut that depends on n alone
//     (never on the grid): every slab's partial sums are formed in one fixed order and stored apart, and a fold
//     adds the slabs in index order.  The grid only decides which workgroup computes which slab, so a capped
//     grid (max_grid) gives the same bits.  ipt grows with n so that there are never more than MAP_MAX_SLABS;
//   * equalisation (histogram and interpolation): MAP_BLOCK rows a trip, grid capped at MAP_MAX_GRID.
// The workspace holds the slabs: slabs * (c*c + c) doubles.
constexpr int MAP_BLOCK = 256;
constexpr int MAP_MAX_C = 8;
constexpr int MAP_MAX_BINS = 1024;
constexpr int MAP_PROJ_WAVE_ROWS = 8;
constexpr int MAP_PROJ_ROWS = MAP_PROJ_WAVE_ROWS * (MAP_BLOCK / 64);
constexpr int MAP_MIN_IPT = 4;
constexpr int64_t MAP_MAX_SLABS = 2048;
constexpr int64_t MAP_MAX_GRID = 2048;            // 256 CUs x 8 workgroups of 4 waves
constexpr int64_t MAP_MAX_ROWS = INT64_C(1) << 40;

struct MapPlan {
    bool valid = false;
    int block = MAP_BLOCK;
    int64_t proj_groups = 0;            // row groups of the projection
    unsigned proj_grid = 0;
    int64_t ipt = 0, chunk = 0;         // ICA step: rows per thread and per slab
    int64_t slabs = 0;
    unsigned step_grid = 0;
    int slab_doubles = 0;               // c*c + c
    size_t ws_bytes = 0;
    int64_t eq_blocks = 0;
    unsigned eq_grid = 0;
    // slabs workgroup x computes (x, x + step_grid, ...); rows of slab s
    int64_t slabs_of(int64_t x) const { return x < slabs ? (slabs - x + step_grid - 1) / step_grid : 0; }
    int64_t slab_rows(int64_t s, int64_t n) const { return s < slabs ? std::min(chunk, n - s * chunk) : 0; }
};

// max_grid: 0 the plan's choice, g > 0 at most g workgroups a launch (tests of the second trip).
// Invalid: n < 1 or beyond 2^40, c outside 1..MAP_MAX_C, a negative max_grid.
inline MapPlan map_plan(int64_t n, int c, int64_t max_grid = 0) {
    MapPlan p;
    if (n < 1 || n > MAP_MAX_ROWS || c < 1 || c > MAP_MAX_C || max_grid < 0) return p;
    const int64_t cap = max_grid > 0 ? std::min(max_grid, MAP_MAX_GRID) : MAP_MAX_GRID;
    p.proj_groups = (n + MAP_PROJ_ROWS - 1) / MAP_PROJ_ROWS;
    p.proj_grid = (unsigned)std::min(p.proj_groups, cap);
    const int64_t per_slab = (n + MAP_MAX_SLABS - 1) / MAP_MAX_SLABS;
    p.ipt = std::max<int64_t>(MAP_MIN_IPT, (per_slab + MAP_BLOCK - 1) / MAP_BLOCK);
    p.chunk = p.ipt * MAP_BLOCK;
    p.slabs = (n + p.chunk - 1) / p.chunk;
    p.step_grid = (unsigned)std::min(p.slabs, cap);
    p.slab_doubles = c * c + c;
    p.ws_bytes = (size_t)p.slabs * (size_t)p.slab_doubles * sizeof(double);
    p.eq_blocks = (n + MAP_BLOCK - 1) / MAP_BLOCK;
    p.eq_grid = (unsigned)std::min(p.eq_blocks, cap);
    p.valid = true;
    return p;
}

// The neighbour and grid geo priors (neighbor_kernel.h; include/range_neighbors.h).
//   * vote scan: a workgroup of NEIGHBOR_VOTE_BLOCK threads owns a group of G consecutive queries, their int32 count
//     rows (G * C * 4 bytes) in LDS beside NEIGHBOR_QUERY_LDS bytes of parameters a query.  G depends on C alone:
//     as many rows as NEIGHBOR_COUNT_LDS holds, at most NEIGHBOR_MAX_GROUP (4 at C = 8142, 1 at the class cap
//     NEIGHBOR_MAX_CLASSES = 32768, whose row is 128 KB of the CU's 160 KB).  The training points are walked in
//     tiles of NEIGHBOR_BLOCK, dealt round-robin to `chunks` workgroups a group (grid y) when the groups alone do
//     not reach NEIGHBOR_TARGET_WG; every chunk keeps a tile, there are at most NEIGHBOR_MAX_CHUNKS, and the
//     partial count rows (chunks * groups * G * C int32) stay below NEIGHBOR_MAX_WS bytes.  With more than one
//     chunk a fold launch (a workgroup a group) sums them and ranks.
//   * k-th neighbour selection: a workgroup a query (grid-stride), NEIGHBOR_PASSES scans of the training set, one
//     per NEIGHBOR_DIGIT_BITS-bit digit of the 64-bit key from the top (the first digit is the 9 bits left over),
//     a 2^NEIGHBOR_DIGIT_BITS-bin histogram in LDS, then one ordered walk for the last tie.
enum { NEIGHBOR_RADIUS = 0, NEIGHBOR_KNN = 1, NEIGHBOR_CELL = 2, NEIGHBOR_MODES = 3 };
constexpr int NEIGHBOR_BLOCK = 256;                // a tile of training points; the selection's and the packing's workgroup
constexpr int NEIGHBOR_VOTE_BLOCK = 1024;          // the vote scan's and the fold's workgroup: four tiles side by side
constexpr int NEIGHBOR_MAX_GROUP = 8;
constexpr int NEIGHBOR_MAX_CLASSES = 32768;
constexpr size_t NEIGHBOR_COUNT_LDS = 132 * 1024;
constexpr size_t NEIGHBOR_QUERY_LDS = 48;
constexpr int NEIGHBOR_MAX_CHUNKS = 64;
constexpr int64_t NEIGHBOR_TARGET_WG = 1024;
constexpr int64_t NEIGHBOR_MAX_GRID = 1 << 16;
constexpr int64_t NEIGHBOR_MAX_POINTS = (INT64_C(1) << 31) - 1;     // the counts are int32
constexpr int64_t NEIGHBOR_MAX_QUERIES = (INT64_C(1) << 31) - 1;
constexpr size_t NEIGHBOR_MAX_WS = (size_t)1 << 30;
constexpr int NEIGHBOR_DIGIT_BITS = 11;
constexpr int NEIGHBOR_PASSES = (64 + NEIGHBOR_DIGIT_BITS - 1) / NEIGHBOR_DIGIT_BITS;
constexpr int NEIGHBOR_BINS = 1 << NEIGHBOR_DIGIT_BITS;

struct NeighborPlan {
    bool valid = false;
    const char* why = "";
    int block = NEIGHBOR_BLOCK, vote_block = NEIGHBOR_VOTE_BLOCK;
    int group = 0;                      // G
    int64_t groups = 0, n_tiles = 0;
    unsigned grid = 0;                  // workgroups over the groups (grid x), walked grid-stride
    int chunks = 0;                     // grid y
    unsigned fold_grid = 0;             // chunks > 1: workgroups of the fold launch
    size_t lds_bytes = 0;
    size_t ws_ints = 0, ws_bytes = 0;   // chunks > 1: the partial count rows
    unsigned select_grid = 0;           // workgroups of the selection, a query each, walked grid-stride
    size_t select_lds = 0;
    int64_t groups_of(int64_t x) const { return x < groups ? (groups - x + grid - 1) / grid : 0; }
    int64_t tiles_of(int64_t y) const { return y < n_tiles ? (n_tiles - y + chunks - 1) / chunks : 0; }
    // the bit shift of pass p's digit (the passes go from the top digit down)
    static constexpr int shift_of(int pass) { return (NEIGHBOR_PASSES - 1 - pass) * NEIGHBOR_DIGIT_BITS; }
};

// queries a workgroup for C classes whose rows have `entry`-byte entries (0: C outside 1 .. max_classes)
inline int neighbor_group_of(int C, size_t entry, int max_classes) {
    if (C < 1 || C > max_classes) return 0;
    return (int)std::min<size_t>(NEIGHBOR_MAX_GROUP, NEIGHBOR_COUNT_LDS / ((size_t)C * entry));
}
inline int neighbor_group(int C) { return neighbor_group_of(C, 4, NEIGHBOR_MAX_CLASSES); }

// what every scan's plan refuses of B queries, `points` training points or bins (N or M in the text), max_grid and
// chunks, with the plan's `own` refusal (or null) at its place in the order: the reason, or null
inline const char* neighbor_plan_refusal(int64_t B, int64_t points, bool bins, const char* own, int64_t max_grid, int chunks) {
    if (B < 1 || B > NEIGHBOR_MAX_QUERIES) return "B outside 1 .. 2^31 - 1";
    if (points < 1 || points > NEIGHBOR_MAX_POINTS) return bins ? "M outside 1 .. 2^31 - 1" : "N outside 1 .. 2^31 - 1";
    if (own) return own;
    if (max_grid < 0 || chunks < 0) return "max_grid or chunks below 0";
    return nullptr;
}

// the geometry of a vote scan whose LDS rows have `entry`-byte entries and G = `group` rows a workgroup: groups,
// tiles, grids, chunks, LDS and workspace (ws_ints counts entries).  The arguments have been checked.
inline void neighbor_plan_rows(NeighborPlan& p, int64_t B, int64_t N, int C, int64_t max_grid, int chunks, size_t entry, int group) {
    const int64_t cap = max_grid > 0 ? std::min(max_grid, NEIGHBOR_MAX_GRID) : NEIGHBOR_MAX_GRID;
    p.group = group;
    p.groups = (B + p.group - 1) / p.group;
    p.n_tiles = (N + NEIGHBOR_BLOCK - 1) / NEIGHBOR_BLOCK;
    p.grid = (unsigned)std::min(p.groups, cap);
    const size_t row_ints = (size_t)p.groups * (size_t)p.group * (size_t)C;       // of one chunk
    const int64_t want = chunks > 0 ? (int64_t)chunks : (NEIGHBOR_TARGET_WG + p.groups - 1) / p.groups;
    const int64_t fits = std::max<int64_t>(1, (int64_t)(NEIGHBOR_MAX_WS / entry / row_ints));
    p.chunks = (int)std::min(std::min(std::min(want, p.n_tiles), std::min(fits, cap)), (int64_t)NEIGHBOR_MAX_CHUNKS);
    p.lds_bytes = (((size_t)p.group * (size_t)C * entry + 15) & ~(size_t)15) + (size_t)p.group * NEIGHBOR_QUERY_LDS;
    if (p.chunks > 1) {
        p.ws_ints = (size_t)p.chunks * row_ints;
        p.ws_bytes = p.ws_ints * entry;
        p.fold_grid = (unsigned)std::min(p.groups, cap);
    }
    p.select_grid = (unsigned)std::min(B, cap);
    p.select_lds = (size_t)(NEIGHBOR_BINS + NEIGHBOR_BLOCK + 16) * 4;
}

// B queries, N training points, C classes; k: neighbours of the selection (0: none asked for).  max_grid: 0 the
// plan's choice, g > 0 at most g workgroups a launch and grid dimension.  chunks: 0 the plan's choice, n > 0 at
// most n chunks (never more than the tiles, NEIGHBOR_MAX_CHUNKS or what the workspace cap allows).
inline NeighborPlan neighbor_plan(int64_t B, int64_t N, int C, int64_t k, int64_t max_grid = 0, int chunks = 0) {
    NeighborPlan p;
    const char* const own = C < 1 || C > NEIGHBOR_MAX_CLASSES ? "num_classes outside 1 .. 32768 (one count row of LDS)"
                            : k < 0 || k > N                  ? "k outside 1 .. N"
                                                              : nullptr;
    if (const char* why = neighbor_plan_refusal(B, N, false, own, max_grid, chunks)) { p.why = why; return p; }
    neighbor_plan_rows(p, B, N, C, max_grid, chunks, 4, neighbor_group(C));
    p.valid = true;
    return p;
}

// The KDE geo prior (kde_kernel.h): the vote scan's geometry over M bins with uint64 rows - the fixed-point sums of
// the members' weights - so G is half the neighbour priors' (2 at C = 8142, 1 at the class cap KDE_MAX_CLASSES =
// 16384, a row of 128 KB).  A weight w in [0, 1] enters a row as count * rint(w * 2^scale_bits); scale_bits is the
// largest s <= KDE_MAX_SCALE_BITS with total_count * 2^s < 2^62, total_count the sum of the bins' counts (at most
// 2^31 - 1), so that no row - nor the sum of a query's rows - can reach 2^62.
constexpr int KDE_MAX_CLASSES = 16384;
constexpr int KDE_MAX_SCALE_BITS = 52;
constexpr int64_t KDE_MAX_TOTAL = (INT64_C(1) << 31) - 1;

struct KdePlan : NeighborPlan {
    int scale_bits = 0;
};

inline int kde_group(int C) { return neighbor_group_of(C, 8, KDE_MAX_CLASSES); }

// (0: total_count outside 1 .. KDE_MAX_TOTAL)
inline int kde_scale_bits(int64_t total_count) {
    if (total_count < 1 || total_count > KDE_MAX_TOTAL) return 0;
    int bits = 0;                        // total_count < 2^bits
    while ((INT64_C(1) << bits) <= total_count) ++bits;
    return std::min(KDE_MAX_SCALE_BITS, 62 - bits);
}

// B queries, M bins, C classes, total_count the sum of the bins' counts; max_grid and chunks as neighbor_plan's
inline KdePlan kde_plan(int64_t B, int64_t M, int C, int64_t total_count, int64_t max_grid = 0, int chunks = 0) {
    KdePlan p;
    const char* const own = C < 1 || C > KDE_MAX_CLASSES                    ? "num_classes outside 1 .. 16384 (one row of 64-bit sums in LDS)"
                            : total_count < M || total_count > KDE_MAX_TOTAL ? "total count outside M .. 2^31 - 1"
                                                                             : nullptr;
    if (const char* why = neighbor_plan_refusal(B, M, true, own, max_grid, chunks)) { p.why = why; return p; }
    neighbor_plan_rows(p, B, M, C, max_grid, chunks, 8, kde_group(C));
    p.scale_bits = kde_scale_bits(total_count);
    p.valid = true;
    return p;
}

// The cluster map (cluster_kernels.h; include/range_cluster.h): complete-linkage clustering of n unit rows of d
// features through their n x n float64 distance matrix.
//   * normalise: a wave a row, CLUSTER_NORM_ROWS rows a trip of a workgroup of CLUSTER_BLOCK threads;
//   * distances: the GEMM's lower triangle is finished in tiles of CLUSTER_TILE x CLUSTER_TILE, a workgroup a tile
//     of the tile triangle (tj <= ti), which also writes the mirrored tile;
//   * linkage rounds: the row scan takes a workgroup a stale row; the merges walk items of (pair, chunk of
//     CLUSTER_CHUNK columns); the three list kernels (stale rows, reciprocal pairs, deactivation) are one workgroup of
//     CLUSTER_SERIAL_BLOCK threads, thread t owning the rows [t * serial_rows, (t + 1) * serial_rows) so that its
//     lists come out in ascending row order.
// Every grid is capped at CLUSTER_MAX_GRID (or max_grid) workgroups and walks its items grid-stride; no result
// depends on the grid.  The workspace holds the linkage state at the byte offsets below.
constexpr int CLUSTER_BLOCK = 256;
constexpr int CLUSTER_NORM_ROWS = CLUSTER_BLOCK / 64;
constexpr int CLUSTER_NORM_REGS = 32;              // a lane keeps up to 32 entries of its row: rows of d <= 2048 are read once
constexpr int CLUSTER_TILE = 64;
constexpr int CLUSTER_CHUNK = 1024;
constexpr int CLUSTER_SERIAL_BLOCK = 1024;
constexpr int64_t CLUSTER_MAX_GRID = 4096;
constexpr int64_t CLUSTER_MAX_ROWS = INT64_C(1) << 17;     // 2^17 rows: a 137 GB matrix
constexpr int CLUSTER_MAX_D = 1 << 20;

struct ClusterPlan {
    bool valid = false;
    int block = CLUSTER_BLOCK, serial_block = CLUSTER_SERIAL_BLOCK;
    int64_t norm_groups = 0;            // row groups of the normaliser
    unsigned norm_grid = 0;
    int64_t tiles = 0, fin_items = 0;   // tiles a side; tiles of the triangle
    unsigned fin_grid = 0;
    unsigned scan_grid = 0;             // workgroups of the first scan (later ones: min(active rows, cap))
    int64_t chunks = 0;                 // column chunks of a row
    int64_t serial_rows = 0;            // rows a thread of the list kernels owns
    int64_t cap = 0;
    size_t matrix_bytes = 0;            // n * n * 8: the caller's D
    // workspace: bytes from its start
    size_t off_active = 0, off_stale = 0, off_mrow = 0, off_nn = 0, off_nnd = 0, off_list = 0, off_pi = 0, off_pj = 0,
           off_counters = 0, ws_bytes = 0;
    // grid of a launch over `items` work items
    unsigned grid_of(int64_t items) const { return (unsigned)std::max<int64_t>(1, std::min(items, cap)); }
    int64_t items_of(int64_t x, int64_t items, int64_t grid) const { return x < items ? (items - x + grid - 1) / grid : 0; }
};

// Invalid: n outside 1 .. 2^17, d outside 1 .. 2^20, a negative max_grid.  (One row has a plan - the normaliser
// takes it - but no linkage.)
inline ClusterPlan cluster_plan(int64_t n, int64_t d, int64_t max_grid = 0) {
    ClusterPlan p;
    if (n < 1 || n > CLUSTER_MAX_ROWS || d < 1 || d > CLUSTER_MAX_D || max_grid < 0) return p;
    p.cap = max_grid > 0 ? std::min(max_grid, CLUSTER_MAX_GRID) : CLUSTER_MAX_GRID;
    p.norm_groups = (n + CLUSTER_NORM_ROWS - 1) / CLUSTER_NORM_ROWS;
    p.norm_grid = p.grid_of(p.norm_groups);
    p.tiles = (n + CLUSTER_TILE - 1) / CLUSTER_TILE;
    p.fin_items = p.tiles * (p.tiles + 1) / 2;
    p.fin_grid = p.grid_of(p.fin_items);
    p.scan_grid = p.grid_of(n);
    p.chunks = (n + CLUSTER_CHUNK - 1) / CLUSTER_CHUNK;
    p.serial_rows = (n + CLUSTER_SERIAL_BLOCK - 1) / CLUSTER_SERIAL_BLOCK;
    p.matrix_bytes = (size_t)n * (size_t)n * sizeof(double);
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t nb = up((size_t)n), half = up((size_t)(n / 2 + 1) * 4);
    p.off_active = 0;
    p.off_stale = p.off_active + nb;
    p.off_mrow = p.off_stale + nb;
    p.off_nn = p.off_mrow + nb;
    p.off_nnd = p.off_nn + up((size_t)n * 4);
    p.off_list = p.off_nnd + (size_t)n * 8;
    p.off_pi = p.off_list + up((size_t)n * 4);
    p.off_pj = p.off_pi + half;
    p.off_counters = p.off_pj + half;
    p.ws_bytes = p.off_counters + 64;
    p.valid = true;
    return p;
}

// The tile (ti, tj <= ti) of item t of the tile triangle, rows first: t = ti (ti + 1) / 2 + tj.
RANGE_HD void cluster_tile_of(int64_t t, int64_t& ti, int64_t& tj) {
    int64_t r = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((r + 1) * (r + 2) / 2 <= t) ++r;
    while (r * (r + 1) / 2 > t) --r;
    ti = r;
    tj = t - r * (r + 1) / 2;
}

// The cut of a complete-linkage tree.  merges (n - 1, 2) and heights (n - 1) are the device's merge record in
// emission order: pair t joined the clusters that then held rows merges[2t] and merges[2t + 1] at height heights[t].
// The merges are sorted stably by height - parents follow their children: heights are monotone under complete
// linkage, and at equal heights a child was emitted in an earlier round - and
//   * labels (n, may be null): the first n - k sorted merges are applied by union-find and the clusters numbered by
//     first occurrence (the cluster of row 0 is 0, the next new one met going down the rows is 1, ...);
//   * Z (n - 1, 4, may be null): scipy's linkage matrix of all of them - the two cluster ids (a row, or n + s for the
//     cluster sorted merge s made; the smaller first), the height, the new cluster's size.
// False: n < 1, k outside 1 .. n, a row index outside 0 .. n - 1, or a merge inside one cluster.
inline bool cluster_cut(int64_t n, const int32_t* merges, const double* heights, int64_t k, int32_t* labels, double* Z) {
    if (n < 1 || k < 1 || k > n || (n > 1 && (!merges || !heights))) return false;
    const int64_t m = n - 1;
    std::vector<int64_t> order((size_t)m);
    for (int64_t t = 0; t < m; ++t) order[(size_t)t] = t;
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return heights[a] < heights[b]; });
    std::vector<int64_t> parent((size_t)n), id((size_t)n), size((size_t)n, 1);
    for (int64_t i = 0; i < n; ++i) parent[(size_t)i] = id[(size_t)i] = i;
    auto find = [&](int64_t x) {
        int64_t r = x;
        while (parent[(size_t)r] != r) r = parent[(size_t)r];
        while (parent[(size_t)x] != r) { const int64_t nx = parent[(size_t)x]; parent[(size_t)x] = r; x = nx; }
        return r;
    };
    auto number = [&]() {
        std::vector<int32_t> of_root((size_t)n, -1);
        int32_t next = 0;
        for (int64_t i = 0; i < n; ++i) {
            const int64_t r = find(i);
            if (of_root[(size_t)r] < 0) of_root[(size_t)r] = next++;
            labels[i] = of_root[(size_t)r];
        }
    };
    if (labels && n - k == 0) number();
    for (int64_t s = 0; s < m; ++s) {
        const int64_t t = order[(size_t)s];
        const int64_t a = merges[2 * t], b = merges[2 * t + 1];
        if (a < 0 || a >= n || b < 0 || b >= n) return false;
        const int64_t ra = find(a), rb = find(b);
        if (ra == rb) return false;
        if (Z) {
            Z[4 * s + 0] = (double)std::min(id[(size_t)ra], id[(size_t)rb]);
            Z[4 * s + 1] = (double)std::max(id[(size_t)ra], id[(size_t)rb]);
            Z[4 * s + 2] = heights[t];
            Z[4 * s + 3] = (double)(size[(size_t)ra] + size[(size_t)rb]);
        }
        parent[(size_t)rb] = ra;
        size[(size_t)ra] += size[(size_t)rb];
        id[(size_t)ra] = n + s;
        if (labels && s + 1 == n - k) number();
    }
    return true;
}

// The fit of the CSP class head from frozen embeddings (headfit_kernels.h; include/range_headfit.h): one step of the
// reference's supervised stage on `rows` = B + Bg gathered rows - the batch's, then the background's - as, per PANEL
// of whole 32-class tiles, the logit gradient G (rows x panel_cols, the head's tile and chunks: csp_head_plan), a
// fold of the tiles' per-row loss sums, and dW = G^T X with Adam behind it.  The panel is the widest that keeps
// the workspace - the gathered X, G, the panel's per-tile row sums (two kinds), the running row sums - within
// HEADFIT_MAX_WS.  An item of the gradient launch is (row tile, chunk of the panel), of the update (class tile,
// group of HEADFIT_FGROUP features: four waves of two 32-feature tiles); both are walked grid-stride.
constexpr int64_t HEADFIT_MAX_ROWS = 8192;
constexpr size_t HEADFIT_MAX_WS = (size_t)256 << 20;
constexpr int HEADFIT_FGROUP = 256;

struct HeadfitPlan {
    bool valid = false;
    const char* why = "";
    int C = 0, F = 0;
    int64_t rows = 0, row_tiles = 0, max_grid = 0;
    int m_tiles = 0, tile_rows = 0, ld = 0, k_groups = 0, n_tiles = 0, wave_tiles = 0, cols_per_pass = 0;
    int panel_cols = 0, panel_tiles = 0, n_panels = 0, f_groups = 0;
    size_t lds_bytes = 0, packed_floats = 0;
    size_t x_floats = 0, g_floats = 0, part_floats = 0, rowsum_floats = 0, ws_bytes = 0;   // the workspace, in this order
    unsigned row_grid = 0;               // of the per-row kernels (fold)
    unsigned gather_grid = 0, unpack_grid = 0;
    int block = CSP_BLOCK;
    unsigned cap(int64_t items) const { return csp_grid_cap(items, max_grid); }
    // panel p: its first class tile, its tiles
    int panel_first_tile(int p) const { return p * panel_tiles; }
    int panel_n_tiles(int p) const { return std::min(panel_tiles, n_tiles - p * panel_tiles); }
    // the gradient launch of panel p: chunks of cols_per_pass columns, items = row tiles x chunks
    int grad_chunks(int p) const { return (panel_n_tiles(p) + 4 * wave_tiles - 1) / (4 * wave_tiles); }
    int64_t grad_items(int p) const { return row_tiles * grad_chunks(p); }
    unsigned grad_grid(int p) const { return cap(grad_items(p)); }
    void grad_item(int p, int64_t it, int64_t& row_tile, int& chunk) const {
        row_tile = it / grad_chunks(p);
        chunk = (int)(it - row_tile * grad_chunks(p));
    }
    // the local tiles wave `w` computes in chunk `ch` of panel p: the first, and how many (stride 4)
    int wave_first_tile(int ch, int w) const { return ch * 4 * wave_tiles + w; }
    int wave_n_tiles(int p, int ch, int w) const {
        const int t0 = wave_first_tile(ch, w), n = panel_n_tiles(p);
        return n > t0 ? std::min(wave_tiles, (n - t0 + 3) / 4) : 0;
    }
    // the update launch of panel p: items = class tiles x feature groups
    int64_t update_items(int p) const { return (int64_t)panel_n_tiles(p) * f_groups; }
    unsigned update_grid(int p) const { return cap(update_items(p)); }
};

// panel_cols: 0, or a narrower panel than the workspace allows (rounded up to whole tiles) - for tests
inline HeadfitPlan headfit_plan(int C, int F, int64_t rows, int64_t max_grid = 0, int panel_cols = 0) {
    HeadfitPlan p;
    if (F < 1 || F > CSP_MAX_WIDTH) { p.why = "feature width outside 1 .. 1024"; return p; }
    if (C < 1 || C > CSP_MAX_CLASSES) { p.why = "num_classes outside 1 .. 32768"; return p; }
    if (rows < 1 || rows > HEADFIT_MAX_ROWS) { p.why = "B + Bg outside 1 .. 8192"; return p; }
    if (max_grid < 0 || panel_cols < 0) { p.why = "max_grid and panel_cols must be >= 0"; return p; }
    const CspHeadPlan h = csp_head_plan(F, C, C, rows, CSP_HEAD_PROBS);
    p.C = C; p.F = F; p.rows = rows; p.max_grid = max_grid;
    p.m_tiles = h.m_tiles; p.tile_rows = h.tile_rows; p.ld = h.ld; p.k_groups = h.k_groups; p.n_tiles = h.n_tiles;
    p.wave_tiles = h.wave_tiles; p.cols_per_pass = h.cols_per_pass; p.row_tiles = h.row_tiles;
    p.packed_floats = h.packed_floats;
    // X tile, and the labels of its rows
    p.lds_bytes = ((size_t)p.tile_rows * p.ld + (size_t)p.tile_rows) * sizeof(float);
    p.x_floats = (size_t)rows * F;
    p.rowsum_floats = 2 * (size_t)rows;
    // a tile of the panel costs 32 columns of G and two row sums per row
    const size_t fixed = (p.x_floats + p.rowsum_floats) * sizeof(float), per_tile = (size_t)rows * (CSP_NTILE + 2) * sizeof(float);
    int tiles = (int)std::min<size_t>((HEADFIT_MAX_WS - fixed) / per_tile, (size_t)p.n_tiles);
    if (panel_cols) tiles = std::min(tiles, (panel_cols + CSP_NTILE - 1) / CSP_NTILE);
    p.panel_tiles = tiles;
    p.panel_cols = tiles * CSP_NTILE;
    p.n_panels = (p.n_tiles + tiles - 1) / tiles;
    p.g_floats = (size_t)rows * p.panel_cols;
    p.part_floats = 2 * (size_t)tiles * rows;
    p.ws_bytes = (p.x_floats + p.g_floats + p.part_floats + p.rowsum_floats) * sizeof(float);
    p.f_groups = (F + HEADFIT_FGROUP - 1) / HEADFIT_FGROUP;
    p.row_grid = p.cap((rows + CSP_BLOCK - 1) / CSP_BLOCK);
    p.gather_grid = p.cap(((int64_t)p.x_floats + CSP_BLOCK - 1) / CSP_BLOCK);
    p.unpack_grid = p.cap(((int64_t)C * F + CSP_BLOCK - 1) / CSP_BLOCK);
    p.valid = true;
    return p;
}


// The fit of a whole CSP location encoder with its class head (cspfit_kernels.h; include/range_cspfit.h): one step of
// the reference's supervised stage on `rows` = B + Bg locations, layer by layer.  Forward, per layer: Z = X W^T as the
// class head's LOGITS launch (csp_head_plan with the layer's weight in the head's packed layout), then a row launch
// (bias, activation, dropout, skip, LayerNorm - `lpr` = CSP_BLOCK / the encoder's tile rows lanes a row, the
// encoder's own reduction order).  The head is headfit_plan on the embeddings, with dE = G W_c behind every
// panel's logit gradient.  Backward, per layer from the last: a row launch (LayerNorm backward, skip, mask, act'),
// the column sums (db, dgamma, dbeta; one thread a column, rows in order), dX = dZ W (an item: 32 rows x
// CSPFIT_BACK_COLS columns, a wave one 32 x 32 tile) and dW = dZ^T X as the head fit's update launch.
//
// Stored parameters - the same offsets into the weights and Adam's two moments: per layer W in the head's packed
// layout, b, gamma, beta (each padded to whole 32-column tiles; gamma / beta only behind a LayerNorm), then the
// packed class_emb.  Unpacked order (range_cspfit_grad / _params): per layer W (out, in), b, gamma, beta, then
// class_emb (C, num_filts).  Workspace: the features and every layer's output (a layer's input is the one before
// it), every layer's pre-activation Z, two gradient images (ping-pong dY / dX), dZ, dY * xhat, then the head's G,
// tile sums and row sums; at most CSPFIT_MAX_WS, or the shape is refused.
constexpr size_t CSPFIT_MAX_WS = (size_t)512 << 20;
constexpr int CSPFIT_BACK_COLS = 128;
constexpr int CSPFIT_COLSUM_BLOCK = 64;

struct CspfitPlan {
    bool valid = false;
    const char* why = "";
    CspPlan net;                         // csp_plan of the network on `rows` locations: widths, live skips, LayerNorms
    HeadfitPlan head;                    // the class head on (rows, num_filts)
    int64_t rows = 0, max_grid = 0;
    int C = 0, n_layers = 0, widest = 0, lpr = 0, rows_per_wg = 0;
    size_t w_off[CSP_MAX_LAYERS] = {}, b_off[CSP_MAX_LAYERS] = {}, g_off[CSP_MAX_LAYERS] = {}, be_off[CSP_MAX_LAYERS] = {};
    size_t c_off = 0, store_floats = 0;
    size_t uw_off[CSP_MAX_LAYERS] = {}, ub_off[CSP_MAX_LAYERS] = {}, ug_off[CSP_MAX_LAYERS] = {}, ube_off[CSP_MAX_LAYERS] = {};
    size_t uc_off = 0, n_params = 0;
    size_t x_off[CSP_MAX_LAYERS + 1] = {}, z_off[CSP_MAX_LAYERS] = {};   // x_off[l]: layer l's input; [n_layers]: the embeddings
    size_t dy_off[2] = {}, dz_off = 0, dyx_off = 0, g_ws_off = 0, part_off = 0, rowsum_off = 0, ws_floats = 0, ws_bytes = 0;
    size_t lds_bytes = 0;                // the largest of the launches
    unsigned feat_grid = 0, row_grid = 0;
    int block = CSP_BLOCK;
    unsigned cap(int64_t items) const { return csp_grid_cap(items, max_grid); }
    int in(int l) const { return net.layer[l].in; }
    int out(int l) const { return net.layer[l].out; }
    // layer l's forward product: the head's LOGITS launch on (rows, in) x (out, in)^T
    CspHeadPlan fwd(int l) const { return csp_head_plan(in(l), out(l), out(l), rows, CSP_HEAD_LOGITS, max_grid); }
    // layer l's dW = dZ^T X: the head fit's update launch with `out` classes of `in` features (always one panel)
    HeadfitPlan upd(int l) const { return headfit_plan(out(l), in(l), rows, max_grid); }
    // dX = dZ W / dE = G W_c on `cols` output columns: items = 32-row tiles x groups of CSPFIT_BACK_COLS columns
    int64_t back_row_tiles() const { return (rows + 31) / 32; }
    int back_col_groups(int cols) const { return (cols + CSPFIT_BACK_COLS - 1) / CSPFIT_BACK_COLS; }
    int64_t back_items(int cols) const { return back_row_tiles() * back_col_groups(cols); }
    unsigned back_grid(int cols) const { return cap(back_items(cols)); }
    // the column sums of layer l: one thread a (kind, column)
    int colsum_kinds(int l) const { return net.layer[l].layn ? 3 : 1; }
    unsigned colsum_grid(int l) const { return cap(((int64_t)colsum_kinds(l) * out(l) + CSPFIT_COLSUM_BLOCK - 1) / CSPFIT_COLSUM_BLOCK); }
};

inline CspfitPlan cspfit_plan(int kind, int F, int n_layers, const int* widths, bool skip, bool use_layn, int C, int64_t rows,
                              int64_t max_grid = 0, int panel_cols = 0) {
    CspfitPlan p;
    if (rows < 1 || rows > HEADFIT_MAX_ROWS) { p.why = "B + Bg outside 1 .. 8192"; return p; }
    if (max_grid < 0 || panel_cols < 0) { p.why = "max_grid and panel_cols must be >= 0"; return p; }
    p.net = csp_plan(kind, F, n_layers, widths, skip, use_layn, rows, max_grid);
    if (!p.net.valid) { p.why = p.net.why; return p; }
    p.head = headfit_plan(C, p.net.out_width, rows, max_grid, panel_cols);
    if (!p.head.valid) { p.why = p.head.why; return p; }
    p.rows = rows; p.max_grid = max_grid; p.C = C; p.n_layers = n_layers;
    p.lpr = CSP_BLOCK / p.net.tile_rows;
    p.rows_per_wg = p.net.tile_rows;
    size_t off = 0, uoff = 0, ws = 0;
    p.widest = 0;
    p.x_off[0] = ws;
    ws += (size_t)rows * p.net.in0;
    p.lds_bytes = p.head.lds_bytes;
    for (int l = 0; l < n_layers; ++l) {
        const CspLayerPlan& L = p.net.layer[l];
        const CspHeadPlan f = p.fwd(l);
        p.lds_bytes = std::max(p.lds_bytes, f.lds_bytes);
        p.w_off[l] = off; off += f.packed_floats;
        p.b_off[l] = off; off += L.n_pad();
        if (L.layn) { p.g_off[l] = off; p.be_off[l] = off + L.n_pad(); off += 2 * (size_t)L.n_pad(); }
        p.uw_off[l] = uoff; uoff += (size_t)L.out * L.in;
        p.ub_off[l] = uoff; uoff += L.out;
        if (L.layn) { p.ug_off[l] = uoff; p.ube_off[l] = uoff + L.out; uoff += 2 * (size_t)L.out; }
        p.z_off[l] = ws; ws += (size_t)rows * L.out;
        p.x_off[l + 1] = ws; ws += (size_t)rows * L.out;
        p.widest = std::max(p.widest, std::max(L.in, L.out));
    }
    p.c_off = off; off += p.head.packed_floats;
    p.uc_off = uoff; uoff += (size_t)C * p.net.out_width;
    p.store_floats = off;
    p.n_params = uoff;
    for (int i = 0; i < 2; ++i) { p.dy_off[i] = ws; ws += (size_t)rows * p.widest; }
    p.dz_off = ws; ws += (size_t)rows * p.widest;
    p.dyx_off = ws; ws += (size_t)rows * p.widest;
    if (ws * sizeof(float) + HEADFIT_MAX_WS > CSPFIT_MAX_WS) { p.why = "the saved activations of B + Bg rows exceed the 512 MiB workspace"; return p; }
    p.g_ws_off = ws; ws += p.head.g_floats;
    p.part_off = ws; ws += p.head.part_floats;
    p.rowsum_off = ws; ws += p.head.rowsum_floats;
    p.ws_floats = ws;
    p.ws_bytes = ws * sizeof(float);
    p.feat_grid = p.cap((rows * F + CSP_BLOCK - 1) / CSP_BLOCK);
    p.row_grid = p.cap((rows + p.rows_per_wg - 1) / p.rows_per_wg);
    p.valid = true;
    return p;
}

}  // namespace range_host
