// Host-side code of librange_hip.so under sanitizers (CPU only; GPU sanitizers are not available
// on the target pool).  Built by tests/test_host_cpu.py with
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all   (run 1)
//   g++ -std=c++17 -g -O1 -fsanitize=thread                                        (run 2)
// from the very headers the library compiles: host_plan.h (launch plans, encoder slot plan,
// recurrence tables, weight packing) and host_copy.h (the thread pool that fills the caller's
// host array).  Exits non-zero on a failed invariant; a sanitizer report aborts the process.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "../../range_amd/csrc/host_copy.h"
#include "../../range_amd/csrc/host_plan.h"

using namespace range_host;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

static void test_plan_and_packing() {
    std::mt19937_64 rng(7);
    for (int L : {1, 2, 3, 7, 10, 16, 33, 40, 64}) {
        EncoderPlan p;
        CHECK(build_encoder_plan(L, 4, p));
        CHECK((int)p.perm.size() % 8 == 0 && p.slot_base.front() == 0 && p.slot_base.back() == (int)p.perm.size());
        std::vector<int> seen((size_t)L * L, 0);
        for (int f : p.perm) if (f >= 0) { CHECK(f < L * L); ++seen[f]; }
        for (int v : seen) CHECK(v == 1);
        for (int s = 0; s < p.n_slots; ++s) CHECK(p.slot_base[s] % 8 == 0 && p.slot_base[s] < p.slot_base[s + 1]);
        CHECK(p.max_round <= 8 * L + 8 * 4 && p.n_rounds * 4 >= p.n_slots);
        std::vector<double> A, B, S;
        recurrence_tables(L, true, A, B, S);
        CHECK((int)A.size() == L * L && (int)S.size() == L);
        for (double v : S) CHECK(std::isfinite(v) && v > 0.0);
        recurrence_tables(L, false, A, B, S);
        for (int m = 0; m < L; ++m) CHECK((S[m] < 0.0) == (m > 0 && (m & 1)));
        // packing: every weight lands exactly once at the fragment position the kernel reads
        for (int H : {64, 192, 512}) {
            const int K = L * L, Kp = (int)p.perm.size();
            std::vector<double> W((size_t)H * K);
            for (auto& v : W) v = (double)(rng() % 1000003) + 1.0;
            const std::vector<double> P = pack_weights(W.data(), H, K, &p.perm, Kp);
            CHECK(P.size() == (size_t)H * Kp);
            double sw = 0, sp = 0;
            for (double v : W) sw += v;
            for (double v : P) sp += v;
            CHECK(sw == sp);
            const int kp = Kp / 8;
            for (int trial = 0; trial < 200; ++trial) {
                const int n = (int)(rng() % H), kk = (int)(rng() % Kp);
                const int t = n / 16, s = kk / 8, e = (kk % 8) / 4, ln = (n & 15) + 16 * (kk % 4);
                const double got = P[(((size_t)t * kp + s) * 64 + ln) * 2 + e];
                CHECK(got == (p.perm[kk] >= 0 ? W[(size_t)n * K + p.perm[kk]] : 0.0));
            }
        }
    }
}

// the stream-K partition of pass 2: every unit in exactly one range, owner() the inverse of start(),
// and the slab indices w + qtile of a walk unique (what SegWalk / slab_parts rely on)
static void test_streamk_partition() {
    const int64_t Gs[] = {1, 2, 7, 255, 256, 1024};
    const int shapes[][2] = {{1, 4}, {1, 782}, {5, 63}, {79, 782}, {157, 782}, {157, 1024}, {3, 6250}, {1250, 97}};
    for (int64_t G : Gs)
        for (auto& sh : shapes) {
            const int n_qtiles = sh[0], cb = sh[1];
            const int64_t U = (int64_t)n_qtiles * cb;
            CHECK(sk_start(0, U, G) == 0 && sk_start(G, U, G) == U);
            for (int64_t w = 0; w < G; ++w) CHECK(sk_start(w, U, G) <= sk_start(w + 1, U, G));
            // owner(u) = the w with start(w) <= u < start(w + 1)
            const int64_t step = U > 5000 ? 37 : 1;
            for (int64_t u = 0; u < U; u += step) {
                const int64_t w = sk_owner(u, U, G);
                CHECK(w >= 0 && w < G && sk_start(w, U, G) <= u && u < sk_start(w + 1, U, G));
            }
            for (int64_t w = 0; w < G; ++w) {      // (range boundaries exactly)
                const int64_t a = sk_start(w, U, G), b = sk_start(w + 1, U, G);
                if (a < b) CHECK(sk_owner(a, U, G) == w && sk_owner(b - 1, U, G) == w);
            }
            // the walk: segments (w, qtile) in order; slab index w + qtile strictly increases
            int64_t last_slab = -1, covered = 0;
            for (int64_t w = 0; w < G; ++w) {
                int64_t u = sk_start(w, U, G);
                const int64_t u_end = sk_start(w + 1, U, G);
                while (u < u_end) {
                    const int64_t qt = u / cb, bo = u - qt * cb;
                    const int64_t n = std::min<int64_t>(u_end - u, cb - bo);
                    CHECK(n > 0 && w + qt > last_slab && w + qt < G + n_qtiles);
                    last_slab = w + qt;
                    // the reduction's view of this query tile's parts contains this workgroup
                    CHECK(sk_owner(qt * cb, U, G) <= w && w <= sk_owner((qt + 1) * cb - 1, U, G));
                    covered += n;
                    u += n;
                }
            }
            CHECK(covered == U);
        }
    for (int n_blocks : {4, 63, 782, 6250})
        for (int n_cols : {1, 2, 3, 7}) {
            CHECK(sk_col_begin(0, n_blocks, n_cols) == 0 && sk_col_begin(n_cols, n_blocks, n_cols) == n_blocks);
            for (int c = 0; c < n_cols; ++c) CHECK(sk_col_begin(c, n_blocks, n_cols) <= sk_col_begin(c + 1, n_blocks, n_cols));
        }
}

static void test_choose_splits() {
    for (int qt : {1, 2, 16, 79, 157, 1563})
        for (int nb : {1, 3, 4, 64, 782, 3125, 6250})
            for (int per_cu : {1, 4})
                for (int cap : {1, 16, 128, 2048}) {
                    const int ns = choose_splits(qt, nb, 256, per_cu, cap, 0.002);
                    CHECK(ns >= 1 && ns <= std::max(1, std::min(cap, nb / 4 > 0 ? nb / 4 : 1)));
                }
    CHECK(choose_splits(157, 6250, 256, 1, 32, 0.0014) == 13);   // the bench geometry
}

static void test_encoder_split() {
    for (int H : {64, 128, 192, 256, 320, 384, 512})
        for (int n_slots : {1, 2, 4, 6, 9, 21})
            for (long long tiles : {1LL, 2LL, 16LL, 40LL, 79LL, 113LL, 128LL, 129LL, 157LL, 1000LL}) {
                int S = -1, KP = -1;
                choose_encoder_split(256, n_slots, H, tiles, S, KP);
                CHECK(S >= 1 && KP >= 1 && (S * KP == 1 || tiles * S * KP <= 256));
                CHECK(KP == 1 || n_slots / KP >= 3 || KP <= n_slots / 3);
                if (S * KP > 1) CHECK(H % S == 0 && (H / S == 64 || H / S == 128 || H / S == 256 || H / S == 512));
            }
    int S, KP;
    choose_encoder_split(256, 21, 512, 79, S, KP);   // a 1 250-query rank of an 8-GPU strong-scaling step
    CHECK(S == 1 && KP == 3);
    choose_encoder_split(256, 21, 512, 1, S, KP);    // one tile
    CHECK(S * KP == 56 && KP == 7);
    choose_encoder_split(256, 21, 512, 157, S, KP);  // more tiles than half the CUs: no split
    CHECK(S == 1 && KP == 1);
    choose_encoder_split(256, 21, 384, 10, S, KP);   // a width without part kernels
    CHECK(S == 1 && KP == 1);
}

static void test_copy_pool() {
    std::mt19937_64 rng(11);
    for (int threads : {1, 3, 8}) {
        HostCopyPool pool(threads);
        for (size_t bytes : {(size_t)0, (size_t)1, (size_t)4095, (size_t)1 << 20, ((size_t)1 << 20) + 7,
                             (size_t)10485760 + 13, (size_t)33 << 20}) {
            std::vector<unsigned char> src(bytes + 64), dst(bytes + 64, 0xEE);
            for (auto& v : src) v = (unsigned char)rng();
            pool.copy(dst.data() + 32, src.data() + 17, bytes);          // unaligned on purpose
            CHECK(std::memcmp(dst.data() + 32, src.data() + 17, bytes) == 0);
            for (int i = 0; i < 32; ++i) CHECK(dst[i] == 0xEE && dst[32 + bytes + i] == 0xEE);   // nothing beyond
        }
        // jobs back to back reuse the workers
        std::vector<int> hits(threads, 0);
        for (int rep = 0; rep < 50; ++rep) pool.run([&](int t, int n) { CHECK(n == threads); ++hits[t]; });
        for (int v : hits) CHECK(v == 50);
    }
    // several callers at once on ONE pool (Python threads around ctypes calls): every copy complete
    {
        HostCopyPool pool(4);
        const size_t bytes = ((size_t)3 << 20) + 5;
        std::vector<std::thread> callers;
        std::vector<int> ok(6, 0);
        for (int c = 0; c < 6; ++c)
            callers.emplace_back([&, c] {
                std::vector<unsigned char> src(bytes, (unsigned char)(c + 1)), dst(bytes, 0);
                for (int rep = 0; rep < 8; ++rep) {
                    std::fill(dst.begin(), dst.end(), 0);
                    pool.copy(dst.data(), src.data(), bytes);
                    if (std::memcmp(dst.data(), src.data(), bytes) != 0) return;
                }
                ok[c] = 1;
            });
        for (auto& t : callers) t.join();
        for (int v : ok) CHECK(v == 1);
    }
}

// hidden widths without a kernel run zero-padded as the next width that has one; the cuts of the
// numpy contract stay inside the batch whatever part sizes they are given
static void test_padding_and_host_parts() {
    for (int h = -3; h <= 1100; ++h) {
        const int k = kernel_hidden_width(h);
        if (h < 1 || h > 1024) { CHECK(k == 0); continue; }
        CHECK(k >= h && (k == 768 || k == 1024 || (k <= 512 && k % 64 == 0)));
        CHECK(k - h < 256 && (h % 64 != 0 || h > 512 || k == h) && kernel_hidden_width(k) == k);
    }
    std::mt19937_64 rng(11);
    for (int trial = 0; trial < 50; ++trial) {
        const int n = 1 + (int)(rng() % 70), kin = 1 + (int)(rng() % 90), np = n + (int)(rng() % 40), kp = kin + (int)(rng() % 40);
        std::vector<double> W((size_t)n * kin);
        for (auto& v : W) v = (double)(rng() % 9973) + 1.0;
        const std::vector<double> P = pad_weights(W.data(), n, kin, np, kp);
        CHECK(P.size() == (size_t)np * kp);
        for (int r = 0; r < np; ++r)
            for (int c = 0; c < kp; ++c)
                CHECK(P[(size_t)r * kp + c] == (r < n && c < kin ? W[(size_t)r * kin + c] : 0.0));
    }
    const std::vector<std::vector<int64_t>> tails = {{4096, 512}, {4096, 1}, {1}, {64}, {5000, 5000, 5000}, {100000}, {}, {63, 63, 63},
                                                     {2048, 256}, {1, 1, 1, 1}};
    for (int64_t B : {(int64_t)4096, (int64_t)4097, (int64_t)10000, (int64_t)16384, (int64_t)5000})
        for (const auto& t : tails) {
            const std::vector<int64_t> cuts = host_part_cuts(B, t, 64);
            CHECK(cuts.size() >= 2 && cuts.front() == 0 && cuts.back() == B);
            for (size_t i = 1; i < cuts.size(); ++i) CHECK(cuts[i] > cuts[i - 1]);
            for (size_t i = 1; i + 1 < cuts.size(); ++i) CHECK(cuts[i] % 64 == 0 && cuts[i] < B);
        }
    const std::vector<int64_t> d = host_part_cuts(10000, {4096, 512}, 64);          // the default of range_forward_host
    CHECK(d.size() == 4 && d[1] == 5440 && d[2] == 9536);
}

// ---- the launch plans (host_plan.h): the cases the comments of the plans state, and invariants over
// a sweep of sizes.  The constants are the kernel headers' (engine_ctx.h: PLAN_CONSTS).
static const PlanConsts KC{/*qtile*/ 64, /*blk*/ 16, /*val_dim*/ 1024, /*max_topk*/ 16, /*p1_wg_per_cu*/ 4, /*enc_qtile*/ 32,
                           /*topks_wl*/ 8, /*tg_qblock*/ 256, /*tg_wg_per_cu*/ 2, /*tg_cap_l*/ 32};
static const int CU_COUNTS[] = {64, 80, 104, 128, 208, 256, 304};

static std::vector<int64_t> batch_sweep() {
    std::vector<int64_t> v;
    for (int64_t b = 1; b <= 20000; b += (b < 700 ? 1 : 7)) v.push_back(b);
    for (int64_t b : {2048, 2049, 4096, 4097, 5376, 5377, 8192, 8193, 10000, 12289, 13568, 13569, 16384, 16385, 20000}) v.push_back(b);
    return v;
}

static void check_encoder_split_plan(const EncSplitPlan& s, int n_cu, int H, int64_t B) {
    CHECK(s.tiles >= 1 && (int64_t)s.tiles * 16 >= B && (int64_t)(s.tiles - 1) * 16 < B);
    CHECK(s.S * s.KP > 1 && s.grid == s.tiles * s.S * s.KP && s.grid >= 1 && s.tiles * s.S * s.KP <= n_cu);
    CHECK(split_width_ok(H, s.S) && s.part_cols * s.S == H);
    CHECK(s.h1_doubles >= (size_t)s.KP * s.tiles * 16 * H && s.tile_doubles >= (size_t)s.tiles * 16 * H);
    if (s.one_launch) {
        CHECK(s.tiles <= 128);                   // the phase counters: 256 words per tile, 128 tiles allocated
        CHECK(s.rest_from == 1 && s.n_parts2 * s.part2_cols == H);
        CHECK(s.part2_cols == 64 || s.part2_cols == 128 || s.part2_cols == 256);
    } else if (s.S2 > 1) {
        CHECK(s.tiles * s.S2 <= n_cu && s.n_parts2 == s.S2 && s.part2_cols * s.S2 == H && s.rest_from == 1);
        CHECK(s.part2_cols == 64 || s.part2_cols == 128 || s.part2_cols == 256);
    } else {
        CHECK(s.rest_from == 0);
    }
}

static void test_encoder_plan() {
    // the benchmark's encoder: L = 40 (21 slots), hidden 512, two hidden layers; 256 CUs
    {
        const EncLaunchPlan p = plan_encoder(256, 21, 512, 2, true, true, 10000, 32);
        // 10 000 queries = 256 workgroups of 32 + a split tail of 113 tiles
        CHECK(p.main_B == 8192 && p.n_wg32 == 256 && p.grid == 256 && p.split_B == 1808);
        CHECK(p.split.tiles == 113 && p.split.S == 1 && p.split.KP == 2 && p.split.grid == 226);
        CHECK(p.split.one_launch && p.split.part2_cols == 256 && p.split.n_parts2 == 2);
        // RANGE_ENC_SPLIT=0: 256 x 32 + 113 x 16 in one launch
        const EncLaunchPlan q = plan_encoder(256, 21, 512, 2, false, true, 10000, 32);
        CHECK(q.main_B == 10000 && q.split_B == 0 && q.n_wg32 == 256 && q.grid == 256 + 113);
        // RANGE_ENC_FUSED=0: the tail as separate launches, the second layer over 2 parts per tile
        const EncLaunchPlan r = plan_encoder(256, 21, 512, 2, true, false, 10000, 32);
        CHECK(r.split_B == 1808 && !r.split.one_launch && r.split.S2 == 2 && r.split.part2_cols == 256);
    }
    // 4 097 .. 5 376 queries: a round of 16-query workgroups plus a split tail
    for (int64_t B = 4097; B <= 5376; ++B) {
        const EncLaunchPlan p = plan_encoder(256, 21, 512, 2, true, true, B, 32);
        CHECK(p.main_B == 4096 && p.n_wg32 == 0 && p.grid == 256 && p.split_B == B - 4096 && p.split.S * p.split.KP > 1);
    }
    {
        const EncLaunchPlan p = plan_encoder(256, 21, 512, 2, true, true, 5377, 32);   // beyond: workgroups of 32
        CHECK(p.split_B == 0 && p.n_wg32 == 169 && p.grid == 169);
        const EncLaunchPlan q = plan_encoder(256, 21, 512, 2, true, true, 16, 32);     // one tile: 56 workgroups, one launch
        CHECK(q.main_B == 0 && q.split_B == 16 && q.split.grid == 56 && q.split.KP == 7 && q.split.one_launch &&
              q.split.part2_cols == 64);
        const EncLaunchPlan w = plan_encoder(256, 21, 1024, 2, true, true, 10000, 32); // wide: 16-query workgroups only
        CHECK(w.main_B == 10000 && w.n_wg32 == 0 && w.grid == 625);
    }
    const int shapes[][3] = {{21, 512, 2}, {6, 64, 2}, {21, 256, 1}, {9, 384, 3}, {21, 1024, 2}, {1, 128, 2}};   // slots, H, layers
    const std::vector<int64_t> Bs = batch_sweep();
    for (int n_cu : CU_COUNTS)
        for (auto& sh : shapes)
            for (int fused = 0; fused < 2; ++fused)
                for (int64_t B : Bs) {
                    const int H = sh[1];
                    const EncLaunchPlan p = plan_encoder(n_cu, sh[0], H, sh[2], true, fused != 0, B, 32);
                    CHECK(p.main_B >= 0 && p.split_B >= 0 && p.main_B + p.split_B == B);
                    if (p.main_B > 0) {
                        // workgroups [0, n_wg32) take 32 queries, the rest 16: all queries, no idle workgroup
                        const int64_t cover = (int64_t)32 * p.n_wg32 + (int64_t)16 * (p.grid - p.n_wg32);
                        CHECK(p.grid >= 1 && p.n_wg32 >= 0 && p.n_wg32 <= p.grid && cover >= p.main_B);
                        CHECK(cover - p.main_B < (p.n_wg32 == p.grid ? 32 : 16));
                        CHECK(H <= 512 || p.n_wg32 == 0);
                    }
                    if (p.split_B > 0) check_encoder_split_plan(p.split, n_cu, H, p.split_B);
                    if (p.main_B > 0 && p.split_B > 0) {
                        // what runs in front of a split tail is a main launch alone
                        const EncLaunchPlan m = plan_encoder(n_cu, sh[0], H, sh[2], true, fused != 0, p.main_B, 32);
                        CHECK(m.split_B == 0 && m.main_B == p.main_B && m.n_wg32 == p.n_wg32 && m.grid == p.grid);
                    }
                    const EncLaunchPlan off = plan_encoder(n_cu, sh[0], H, sh[2], false, fused != 0, B, 32);
                    CHECK(off.split_B == 0 && off.main_B == B);
                }
}

static void test_pass_plans() {
    // the bench geometry: 10 000 queries against 100 000 rows on 256 CUs
    {
        const Pass2Plan p = plan_pass2(256, 100000, 10000, true, KC);
        CHECK(p.n_qtiles == 157 && p.n_blocks == 6250 && p.n_splits == 13 && !p.streamk && p.grid == 157 * 13);
        CHECK(p.sk_groups == 0 && p.sk_cols == 1 && p.slab_floats == (size_t)13 * 10000 * 1024);
        const Pass2Plan q = plan_pass2(256, 50000, 10000, true, KC);       // up to 50 000 rows: stream-K
        CHECK(q.streamk && q.sk_groups == 256 && q.grid == 256 && q.sk_cols == 4);
        CHECK(!plan_pass2(256, 50001, 10000, true, KC).streamk && !plan_pass2(256, 50000, 10000, false, KC).streamk);
        const Pass1Plan a = plan_pass1(256, 100000, 10000, false, 0, KC);
        CHECK(a.n_splits == choose_splits(157, 6250, 256, 4, 128) && a.grid == a.n_splits * 157);
        CHECK(plan_pass1(256, 100000, 256, false, 0, KC).n_splits == choose_splits(4, 6250, 256, 4, 2048));   // few queries: up to 2 048
        CHECK(plan_pass1(256, 100000, 257, false, 0, KC).n_splits == choose_splits(5, 6250, 256, 4, 128));
        CHECK(plan_pass1(256, 100000, 256, true, 0, KC).n_splits <= 256 && plan_pass1(256, 100000, 257, true, 0, KC).n_splits <= 16);
        CHECK(plan_pass1(256, 100000, 10000, false, 7, KC).n_splits == 7 && plan_pass1(256, 100, 10000, false, 7, KC).n_splits == 1);
    }
    const int64_t rows_sweep[] = {1, 3, 15, 16, 17, 63, 64, 65, 1000, 1023, 12500, 16384, 16385, 32769, 49999, 50000, 50001, 100000, 250000, 1000000};
    std::vector<int64_t> Bs;
    for (int64_t b : batch_sweep()) if (b < 300 || b % 13 == 0 || b % 64 < 2 || b > 19990) Bs.push_back(b);
    for (int n_cu : CU_COUNTS)
        for (int64_t n_rows : rows_sweep)
            for (int64_t B : Bs) {
                const int n_blocks = (int)((n_rows + 15) / 16), n_qtiles = (int)((B + 63) / 64);
                for (int topk_scan = 0; topk_scan < 2; ++topk_scan) {
                    const Pass1Plan a = plan_pass1(n_cu, n_rows, B, topk_scan != 0, 0, KC);
                    CHECK(a.n_blocks == n_blocks && a.n_qtiles == n_qtiles && a.n_splits >= 1 && a.n_splits <= std::max(1, n_blocks / 4));
                    CHECK(a.grid == a.n_splits * a.n_qtiles && a.grid >= 1 && a.part_floats == (size_t)a.n_splits * B * 4);
                    CHECK(a.merge_by_wave == (a.n_splits > 32));
                    CHECK(a.topk_slots * 16 >= B && a.topk_chunks >= 1 && a.topk_chunks <= 64 && a.topk_chunks <= std::max(1, n_blocks / 32));
                }
                for (int allow = 0; allow < 2; ++allow) {
                    const Pass2Plan p = plan_pass2(n_cu, n_rows, B, allow != 0, KC);
                    CHECK(p.n_blocks == n_blocks && p.n_qtiles == n_qtiles && p.grid >= 1);
                    CHECK(p.n_splits >= 1 && p.n_splits <= std::max(1, n_blocks / 4));
                    CHECK(p.streamk == (allow && n_rows <= 50000));
                    if (!p.streamk) {
                        // one workgroup per (split, query tile); split p of query q at row p B + q
                        CHECK(p.grid == p.n_splits * n_qtiles && p.sk_groups == 0 && p.sk_cols == 1);
                        CHECK(p.slab_floats >= (size_t)p.n_splits * B * 1024);
                        continue;
                    }
                    const int64_t G = p.sk_groups;
                    CHECK(p.grid == G && G >= 1 && G <= n_cu && p.sk_cols >= 1 && p.sk_cols <= n_blocks);
                    int64_t max_slab = -1;
                    for (int c = 0; c < p.sk_cols; ++c) {
                        const int64_t cb = sk_col_begin(c + 1, n_blocks, p.sk_cols) - sk_col_begin(c, n_blocks, p.sk_cols);
                        CHECK(cb >= 1 && cb * 16 <= 16384 + 16 * p.sk_cols);
                        const int64_t U = (int64_t)n_qtiles * cb;
                        // every (query tile, block) unit of the column in exactly one workgroup's range
                        int64_t covered = 0;
                        for (int64_t w = 0; w < G; ++w) {
                            const int64_t u0 = sk_start(w, U, G), u1 = sk_start(w + 1, U, G);
                            CHECK(u0 == covered && u1 >= u0);
                            covered = u1;
                            if (u1 > u0) {
                                CHECK(sk_owner(u0, U, G) == w && sk_owner(u1 - 1, U, G) == w);
                                max_slab = std::max(max_slab, (int64_t)c * (G + n_qtiles) + w + (u1 - 1) / cb);
                            }
                        }
                        CHECK(covered == U);
                    }
                    CHECK((size_t)(max_slab + 1) * 64 * 1024 <= p.slab_floats);
                }
            }
}

static void test_small_and_topk_plans() {
    // up to 32 queries: the one-pass route, one or two query tiles per workgroup
    CHECK(plan_forward_small(256, 100000, 16, KC).nq == 1 && plan_forward_small(256, 100000, 17, KC).nq == 2);
    CHECK(plan_forward_small(256, 100000, 32, KC).nq == 2 && plan_forward_small(256, 100000, 1, KC).nq == 1);
    CHECK(plan_forward_small(256, 100000, 16, KC).n_wg == 256 && plan_forward_small(256, 100, 16, KC).n_wg == 7);
    // the top-k: more than 256 queries take the GEMM route only with the bf16 prefilter on, at least 64
    // bank blocks and a key norm a power of two can scale
    {
        const TopkPlan g = plan_topk(256, 100000, 10000, 1.0001f, true, true, true, false, 5, KC);
        CHECK(g.gemm && g.n_qblocks == 40 && g.n_splits == 12 && g.grid == 480 && g.tile_stride == 5 && g.key_e2 == 1);
        CHECK(!plan_topk(256, 100000, 256, 1.0001f, true, true, true, false, 5, KC).gemm);
        CHECK(plan_topk(256, 100000, 257, 1.0001f, true, true, true, false, 5, KC).gemm);
        CHECK(!plan_topk(256, 100000, 257, 1.0001f, true, false, true, false, 5, KC).gemm);    // RANGE_TOPKS_KEYS=f32
        CHECK(!plan_topk(256, 100000, 257, 1.0001f, false, true, true, false, 5, KC).gemm);    // RANGE_TOPK_GEMM=0
        CHECK(!plan_topk(256, 100000, 257, 1.0001f, true, true, true, true, 5, KC).gemm);      // RANGE_TOPKS_FORCE_EXACT=1
        CHECK(!plan_topk(256, 1008, 257, 1.0001f, true, true, true, false, 5, KC).gemm);       // 63 blocks
        CHECK(plan_topk(256, 1009, 257, 1.0001f, true, true, true, false, 5, KC).gemm);        // 64 blocks
        CHECK(!plan_topk(256, 100000, 257, 0.f, true, true, true, false, 5, KC).gemm);         // all-zero keys
        CHECK(!plan_topk(256, 100000, 257, 1e-35f, true, true, true, false, 5, KC).gemm);      // out of fp16's reach
        CHECK(!plan_topk(256, 100000, 257, INFINITY, true, true, true, false, 5, KC).gemm);
        CHECK(!plan_topk(256, 100000, 60001, 1.0001f, true, true, true, false, 5, KC).gemm);
        const TopkPlan s16 = plan_topk(256, 100000, 16, 1.0001f, true, true, true, false, 5, KC);
        CHECK(!s16.gemm && s16.G == 1 && s16.n_wg == 256 && s16.fused);
        const TopkPlan s256 = plan_topk(256, 100000, 256, 1.0001f, true, true, true, false, 5, KC);
        CHECK(s256.G == 2 && s256.fused && !plan_topk(256, 100000, 257, 1.0001f, false, true, true, false, 5, KC).fused);
        CHECK(!plan_topk(256, 100000, 16, 1.0001f, true, true, false, false, 5, KC).fused);    // RANGE_TOPKS_FUSED=0
    }
    const int64_t rows_sweep[] = {1, 16, 17, 63, 64, 1000, 1008, 1009, 1024, 12500, 50000, 100000, 1000000};
    for (int n_cu : CU_COUNTS)
        for (int64_t n_rows : rows_sweep)
            for (int64_t B : batch_sweep()) {
                const SmallPlan sp = plan_forward_small(n_cu, n_rows, std::min<int64_t>(B, 32), KC);
                CHECK(sp.n_wg >= 1 && sp.n_wg <= n_cu && sp.n_wg <= std::max(1, sp.n_blocks) && sp.qcap >= std::min<int64_t>(B, 32));
                CHECK(sp.o_floats >= (size_t)sp.n_wg * 2 * sp.qcap * 1024 && sp.z_floats >= (size_t)sp.n_wg * sp.qcap * 2);
                for (int sample : {1, 5, 16}) {
                    const TopkPlan t = plan_topk(n_cu, n_rows, B, 1.0001f, true, true, true, false, sample, KC);
                    CHECK(t.n_groups * 16 >= B && t.n_wg >= 1 && t.n_wg <= std::min(n_cu, 256) && (t.G == 1 || t.G == 2));
                    CHECK(!t.fused || B <= t.n_wg);
                    CHECK(t.cand_keys >= (size_t)t.n_groups * 16 * t.n_wg * 8 && t.cand_dmax >= (size_t)t.n_groups * 16 * t.n_wg);
                    if (!t.gemm) continue;
                    CHECK(B > 256 && t.n_blocks >= 64 && (int64_t)t.n_qblocks * 256 >= B && t.n_splits >= 4 && t.n_splits <= 64);
                    CHECK(t.grid == t.n_qblocks * t.n_splits && t.grid >= 1 && t.n_splits <= t.n_blocks / 8);   // >= 8 tiles per split
                    CHECK(t.tile_stride >= 1 && t.tile_stride <= sample);
                }
            }
}

int main() {
    test_padding_and_host_parts();
    test_plan_and_packing();
    test_choose_splits();
    test_streamk_partition();
    test_encoder_split();
    test_encoder_plan();
    test_pass_plans();
    test_small_and_topk_plans();
    test_copy_pool();
    std::puts("host_sanitize ok");
    return 0;
}
