// The location encoder's launch plan (range_amd/csrc/host_plan.h: plan_encoder, plan_encoder_split,
// choose_encoder_split, build_encoder_plan) over its whole envelope, on the CPU.
//
//   enc_sweep_plan            query mode: for every line "n_cu L hidden layers split fused B" on stdin, one line of
//                             key=value fields with what the plan decides (tests/test_enc_sweep_cpu.py and
//                             tests/test_gpu_enc_sweep.py read which kernel tables a case reaches from it)
//   enc_sweep_plan --sweep    L = 1..64 x every kernel width x 1..7 hidden layers x the batch sizes below x both
//                             switches: the invariants the kernels rely on.  Built with g++ under AddressSanitizer /
//                             UndefinedBehaviorSanitizer by tests/test_enc_sweep_cpu.py.
//   enc_sweep_plan --reach    the same sweep at 256 CUs: the table entries any plan reaches, one "TABLE nt" per line
//
// The LDS sizes restate range_set_encoder / range_set_sh_table (encoder_host.h, which needs HIP);
// tests/test_enc_sweep_cpu.py compares the two texts.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../range_amd/csrc/host_plan.h"

using namespace range_host;

#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) {                                                                                \
            std::printf("FAILED line %d: %s  (n_cu=%d L=%d H=%d layers=%d split=%d fused=%d B=%lld)\n", \
                        __LINE__, #cond, g_cu, g_L, g_H, g_layers, g_split, g_fused, (long long)g_B);  \
            return 1;                                                                                 \
        }                                                                                             \
    } while (0)

static int g_cu, g_L, g_H, g_layers, g_split, g_fused;
static int64_t g_B;

constexpr int QTILE = 32;             // encoder_kernel.h: ENC_QTILE
constexpr int SLOTS_PER_ROUND = 4;    // encoder_kernel.h: ENC_SLOTS_PER_ROUND
constexpr size_t LDS_CAP = 160 * 1024;

// range_set_encoder: lds_main (doubles) and lds_bytes; range_set_sh_table: + the power table
static int lds_main_doubles(const EncoderPlan& plan, int H) { return (H > 512 ? 16 : QTILE) * std::max(plan.max_round, H); }
static size_t lds_bytes(const EncoderPlan& plan, int H) { return (size_t)(lds_main_doubles(plan, H) + 16 * QTILE) * sizeof(double); }
static size_t lds_bytes_table(const EncoderPlan& plan, int H, int L) { return lds_bytes(plan, H) + (size_t)QTILE * L * sizeof(double); }

static const int WIDTHS[] = {64, 128, 192, 256, 320, 384, 448, 512, 768, 1024};
static bool is_part_width(int c) { return c == 64 || c == 128 || c == 256 || c == 512; }

typedef std::set<std::pair<std::string, int>> Reach;

// the table entries a plan launches (encoder_host.h: launch_encoder, launch_encoder_split)
static void reach_of(const EncLaunchPlan& p, int H, Reach& r, bool* main32 = nullptr, bool* main16 = nullptr) {
    if (p.main_B > 0) {
        r.insert({"ENC_MAIN", H / 64});
        if (main32 && p.n_wg32 > 0) *main32 = true;
        if (main16 && p.grid > p.n_wg32) *main16 = true;
    }
    if (p.split_B > 0) {
        const EncSplitPlan& sp = p.split;
        if (sp.one_launch) {
            r.insert({"ENC_TILE", sp.part_cols / 64});
        } else {
            r.insert({"ENC_L1_PART", sp.part_cols / 64});
            if (sp.S2 > 1) r.insert({"ENC_L2_PART", sp.part2_cols / 64});
            r.insert({"ENC_REST", H / 64});
        }
    }
}

static int check_slot_plan(int L, const EncoderPlan& plan) {
    g_L = L;
    const int Kp = (int)plan.perm.size();
    CHECK(plan.n_slots == (L == 1 ? 1 : L / 2 + 1));
    CHECK(plan.n_rounds == (plan.n_slots + SLOTS_PER_ROUND - 1) / SLOTS_PER_ROUND);
    CHECK((int)plan.slot_base.size() == plan.n_slots + 1 && plan.slot_base[0] == 0 && plan.slot_base[plan.n_slots] == Kp);
    CHECK(Kp % 8 == 0 && Kp >= L * L);
    std::vector<int> seen((size_t)L * L, 0);
    for (int f : plan.perm) {
        CHECK(f >= -1 && f < L * L);
        if (f >= 0) seen[(size_t)f] += 1;
    }
    for (int v : seen) CHECK(v == 1);
    for (int s = 0; s < plan.n_slots; ++s) {
        CHECK(plan.slot_base[s] % 8 == 0 && plan.slot_base[s + 1] > plan.slot_base[s]);
        // slot s holds the orders {s, L - s} (one of them when they coincide or s = 0), degree by degree, cos before sin
        const int m_a = s, m_b = (s > 0 && L - s > s) ? L - s : -1;
        int pos = plan.slot_base[s];
        for (int m : {m_a, m_b}) {
            if (m < 0) continue;
            for (int l = m; l < L; ++l) {
                CHECK(plan.perm[(size_t)pos++] == l * l + l + m);
                if (m > 0) CHECK(plan.perm[(size_t)pos++] == l * l + l - m);
            }
        }
        CHECK(plan.slot_base[s + 1] - pos >= 0 && plan.slot_base[s + 1] - pos < 8);
        for (; pos < plan.slot_base[s + 1]; ++pos) CHECK(plan.perm[(size_t)pos] == -1);
    }
    for (int r = 0; r < plan.n_rounds; ++r) {
        const int s1 = std::min((r + 1) * SLOTS_PER_ROUND, plan.n_slots);
        CHECK(plan.slot_base[s1] - plan.slot_base[r * SLOTS_PER_ROUND] <= plan.max_round);
    }
    return 0;
}

// the feature rows a workgroup of MODE 1 writes into LDS: K part `kpart` of KP walks its slots four at a time from
// ITS first slot (encoder_kernel.h: encoder_body), 16 queries each
static int check_kpart_rounds(const EncoderPlan& plan, int KP, int lds_main) {
    for (int kpart = 0; kpart < KP; ++kpart) {
        const int ks0 = (plan.n_slots * kpart) / KP, ks1 = (plan.n_slots * (kpart + 1)) / KP;
        CHECK(ks1 - ks0 >= (KP > 1 ? 3 : 1));
        for (int s = ks0; s < ks1; s += SLOTS_PER_ROUND) {
            const int span = plan.slot_base[std::min(s + SLOTS_PER_ROUND, ks1)] - plan.slot_base[s];
            CHECK(span >= 8 && span % 8 == 0 && 16 * span <= lds_main);
        }
    }
    return 0;
}

static int check_plan(int n_cu, const EncoderPlan& plan, int L, int H, int layers, bool split, bool fused, int64_t B,
                      const EncLaunchPlan& p) {
    g_cu = n_cu; g_L = L; g_H = H; g_layers = layers; g_split = split; g_fused = fused; g_B = B;
    const int lds_main = lds_main_doubles(plan, H);
    CHECK(p.main_B >= 0 && p.split_B >= 0 && p.main_B + p.split_B == B);
    CHECK(split || p.split_B == 0);
    if (p.main_B > 0) {
        // workgroup b < n_wg32 takes queries [32 b, 32 b + 32), the others 16 each behind them: every 16-query tile
        // of the main part exactly once, no workgroup without a query
        CHECK(p.n_wg32 >= 0 && p.grid >= 1 && p.n_wg32 <= p.grid);
        CHECK(H <= 512 || p.n_wg32 == 0);
        const int64_t tiles = (p.main_B + 15) / 16;
        std::vector<int> seen((size_t)tiles, 0);
        for (int b = 0; b < p.grid; ++b) {
            const int64_t q0 = b < p.n_wg32 ? (int64_t)b * 32 : (int64_t)p.n_wg32 * 32 + (int64_t)(b - p.n_wg32) * 16;
            CHECK(q0 < p.main_B);
            for (int t = 0; t < (b < p.n_wg32 ? 2 : 1); ++t)
                if (q0 + 16 * t < p.main_B) seen[(size_t)(q0 / 16 + t)] += 1;
        }
        for (int v : seen) CHECK(v == 1);
        CHECK(p.split_B == 0 || p.main_B % 16 == 0);       // the tail's tiles start on a tile of the batch
        // LDS: features of a round and the activations, for the workgroup's queries
        const int qt = p.n_wg32 > 0 ? 32 : 16;
        CHECK(qt * plan.max_round <= lds_main && qt * H <= lds_main);
        bool has = false;
        for (int nt : {1, 2, 3, 4, 5, 6, 7, 8, 12, 16}) has = has || nt * 64 == H;
        CHECK(has);
    } else {
        CHECK(p.n_wg32 == 0 && p.grid == 0);
    }
    if (p.split_B > 0) {
        const EncSplitPlan& sp = p.split;
        CHECK(sp.tiles == (int)((p.split_B + 15) / 16) && sp.tiles >= 1);
        CHECK(sp.S >= 1 && sp.KP >= 1 && sp.S * sp.KP > 1 && sp.KP <= 7);
        CHECK(sp.grid == sp.tiles * sp.S * sp.KP && sp.grid <= n_cu);
        CHECK(sp.part_cols * sp.S == H && is_part_width(sp.part_cols));
        CHECK(sp.h1_doubles >= (size_t)sp.KP * sp.tiles * 16 * H && sp.tile_doubles >= (size_t)sp.tiles * 16 * H);
        if (int rc = check_kpart_rounds(plan, sp.KP, lds_main)) return rc;
        CHECK(16 * H <= lds_main);
        // the first launch: workgroup x -> (tile, column part, K part), each exactly once
        std::vector<int> seen((size_t)sp.grid, 0);
        for (int x = 0; x < sp.grid; ++x) {
            const int per_tile = sp.S * sp.KP, tile = x / per_tile, rest = x - tile * per_tile;
            const int part = rest / sp.KP, kpart = rest - part * sp.KP;
            CHECK(tile < sp.tiles && part < sp.S && kpart < sp.KP);
            seen[(size_t)((tile * sp.S + part) * sp.KP + kpart)] += 1;
        }
        for (int v : seen) CHECK(v == 1);
        if (sp.one_launch) {
            CHECK(fused && layers == 2 && H <= 512);
            CHECK(sp.tiles * sp.S * sp.KP <= n_cu);
            CHECK(sp.tiles * 256 <= 128 * 256);            // launch_encoder_split: the counters' workspace
            CHECK(sp.part2_cols == 64 || sp.part2_cols == 128 || sp.part2_cols == 256);
            CHECK(sp.n_parts2 * sp.part2_cols == H && sp.rest_from == 1);
        } else {
            CHECK(sp.S2 == 1 || sp.S2 == 2 || sp.S2 == 4 || sp.S2 == 8);
            if (sp.S2 > 1) {
                CHECK(layers >= 2 && sp.tiles * sp.S2 <= n_cu);
                CHECK(sp.n_parts2 == sp.S2 && sp.part2_cols * sp.S2 == H && sp.rest_from == 1);
                CHECK(sp.part2_cols == 64 || sp.part2_cols == 128 || sp.part2_cols == 256);
            } else {
                CHECK(sp.rest_from == 0);
            }
            bool has = false;
            for (int nt : {1, 2, 4, 6, 8, 12, 16}) has = has || nt * 64 == H;
            CHECK(has);
        }
    }
    return 0;
}

static std::vector<int64_t> sweep_batches() {
    std::vector<int64_t> bs;
    for (int64_t b = 1; b <= 40; ++b) bs.push_back(b);
    for (int64_t c : {256, 512, 2048, 4096, 8192})
        for (int64_t d = -1; d <= 1; ++d) bs.push_back(c + d);
    for (int64_t b : {5376, 5377, 10000, 24653}) bs.push_back(b);
    return bs;
}

static int sweep(bool print_reach) {
    const std::vector<int64_t> batches = sweep_batches();
    Reach reach;
    long long plans = 0;
    size_t lds_max = 0, lds_table_max = 0;
    for (int L = 1; L <= 64; ++L) {
        EncoderPlan plan;
        g_L = L;
        CHECK(build_encoder_plan(L, SLOTS_PER_ROUND, plan));
        if (int rc = check_slot_plan(L, plan)) return rc;
        for (int H : WIDTHS) {
            g_H = H;
            CHECK(kernel_hidden_width(H) == H);
            // what range_set_encoder / range_set_sh_table accept: the whole envelope
            CHECK(lds_bytes(plan, H) <= LDS_CAP && lds_bytes_table(plan, H, L) <= LDS_CAP);
            lds_max = std::max(lds_max, lds_bytes(plan, H));
            lds_table_max = std::max(lds_table_max, lds_bytes_table(plan, H, L));
            for (int n_cu : print_reach ? std::vector<int>{256} : std::vector<int>{256, 304, 64})
                for (int layers = 1; layers <= 7; ++layers)
                    for (int sw = 0; sw < 4; ++sw)
                        for (int64_t B : batches) {
                            const bool split = sw & 1, fused = sw & 2;
                            const EncLaunchPlan p = plan_encoder(n_cu, plan.n_slots, H, layers, split, fused, B, QTILE);
                            if (int rc = check_plan(n_cu, plan, L, H, layers, split, fused, B, p)) return rc;
                            if (n_cu == 256) reach_of(p, H, reach);
                            ++plans;
                        }
        }
    }
    // hidden widths between the kernels' run at the next one; beyond the envelope nothing is planned
    g_L = g_H = 0;
    CHECK(kernel_hidden_width(0) == 0 && kernel_hidden_width(1025) == 0 && kernel_hidden_width(1) == 64);
    CHECK(kernel_hidden_width(600) == 768 && kernel_hidden_width(513) == 768 && kernel_hidden_width(769) == 1024);
    if (print_reach) {
        for (const auto& e : reach) std::printf("%s %d\n", e.first.c_str(), e.second);
        return 0;
    }
    std::printf("enc_sweep_plan ok: %lld plans, lds_max=%zu lds_table_max=%zu\n", plans, lds_max, lds_table_max);
    return 0;
}

static int query() {
    int n_cu, L, hidden, layers, split, fused;
    long long B;
    while (std::scanf("%d %d %d %d %d %d %lld", &n_cu, &L, &hidden, &layers, &split, &fused, &B) == 7) {
        const int H = kernel_hidden_width(hidden);
        EncoderPlan plan;
        if (n_cu < 1 || L < 1 || L > 64 || H == 0 || layers < 1 || B < 1 || !build_encoder_plan(L, SLOTS_PER_ROUND, plan)) {
            std::printf("invalid\n");
            continue;
        }
        const EncLaunchPlan p = plan_encoder(n_cu, plan.n_slots, H, layers, split != 0, fused != 0, B, QTILE);
        if (int rc = check_plan(n_cu, plan, L, H, layers, split != 0, fused != 0, B, p)) return rc;
        const EncSplitPlan& sp = p.split;
        Reach r;
        bool m32 = false, m16 = false;
        reach_of(p, H, r, &m32, &m16);
        std::string tables;
        for (const auto& e : r) tables += (tables.empty() ? "" : ",") + e.first + ":" + std::to_string(e.second);
        std::printf("n_cu=%d L=%d hidden=%d H=%d layers=%d split=%d fused=%d B=%lld main_B=%lld n_wg32=%d grid=%d split_B=%lld "
                    "tiles=%d S=%d KP=%d one_launch=%d S2=%d part_cols=%d part2_cols=%d rest_from=%d split_grid=%d "
                    "n_slots=%d n_rounds=%d max_round=%d kp0=%d lds=%zu lds_table=%zu main32=%d main16=%d tables=%s\n",
                    n_cu, L, hidden, H, layers, split, fused, B, (long long)p.main_B, p.n_wg32, p.grid, (long long)p.split_B,
                    sp.tiles, sp.S, sp.KP, (int)sp.one_launch, sp.S2, p.split_B > 0 ? sp.part_cols : 0, sp.part2_cols,
                    sp.rest_from, sp.grid, plan.n_slots, plan.n_rounds, plan.max_round, (int)plan.perm.size() / 8,
                    lds_bytes(plan, H), lds_bytes_table(plan, H, L), (int)m32, (int)m16, tables.c_str());
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "--sweep")) return sweep(false);
    if (argc > 1 && !std::strcmp(argv[1], "--reach")) return sweep(true);
    return query();
}
