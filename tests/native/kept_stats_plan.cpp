// The launch plan of the statistics from the kept logits (range_amd/csrc/host_plan.h: plan_kept_stats,
// kept_pair_shift) on the CPU, built with g++ under AddressSanitizer / UndefinedBehaviorSanitizer by
// tests/test_temperature_sweep_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <utility>

#include "../../range_amd/csrc/host_plan.h"

using namespace range_host;

#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);             \
            return 1;                                                         \
        }                                                                     \
    } while (0)

int main() {
    // (engine_prims.h / pass1.h / pass1_kept.h: QTILE, BLK, VAL_DIM, MAX_TOPK, P1_WG_PER_CU, ...; KEPT_MAX_PAIRS)
    const PlanConsts K{64, 16, 1024, 16, 4, 32, 8, 128, 2, 64};
    const int MAXP = 8;
    for (int n_cu : {256, 64})
        for (int64_t n_rows : {9, 1000, 20011, 100000, 12500})
            for (int64_t B : {1, 64, 66, 70, 130, 10000}) {
                // the splits are the scan's: plain, forced, forced beyond what the bank allows (the clamp)
                for (int force : {0, 1, 3, 13, 100000}) {
                    const Pass1Plan s = plan_pass1(n_cu, n_rows, B, false, force, K);
                    for (int P : {1, 2, 7, 8, 9, 16, 17, 25}) {
                        const KeptStatsPlan p = plan_kept_stats(n_cu, n_rows, B, P, force, MAXP, K);
                        CHECK(p.n_splits == s.n_splits && p.n_blocks == s.n_blocks && p.n_qtiles == s.n_qtiles);
                        CHECK(p.grid == p.n_splits * p.n_qtiles && p.grid == s.grid);
                        CHECK(p.merge_by_wave == s.merge_by_wave && p.merge_by_wave == (p.n_splits > 32));
                        CHECK(p.n_splits >= 1 && p.n_splits <= (p.n_blocks / 4 > 1 ? p.n_blocks / 4 : 1));
                        if (force > 0) CHECK(p.n_splits == (force < (p.n_blocks / 4 > 1 ? p.n_blocks / 4 : 1) ? force : (p.n_blocks / 4 > 1 ? p.n_blocks / 4 : 1)));
                        // groups: every pair once, in order, at most MAXP per launch, only the last one short
                        CHECK((int)p.groups.size() == (P + MAXP - 1) / MAXP);
                        int next = 0;
                        for (size_t g = 0; g < p.groups.size(); ++g) {
                            CHECK(p.groups[g].first == next && p.groups[g].count >= 1 && p.groups[g].count <= MAXP);
                            if (g + 1 < p.groups.size()) CHECK(p.groups[g].count == MAXP);
                            next += p.groups[g].count;
                        }
                        CHECK(next == P);
                        // workspace: the parts (split, B, 4) of the largest group
                        CHECK(p.part_floats == (size_t)p.n_splits * (size_t)B * 4);
                        CHECK(p.ws_floats == p.part_floats * (size_t)(P < MAXP ? P : MAXP));
                    }
                }
            }
    // the bench shape: what the scan of 10 000 queries against 100 000 rows chooses
    CHECK(plan_kept_stats(256, 100000, 10000, 5, 0, MAXP, K).n_splits == plan_pass1(256, 100000, 10000, false, 0, K).n_splits);
    CHECK(plan_kept_stats(256, 100000, 10000, 0, 0, MAXP, K).groups.empty());
    // the shift of a pair: plan_temperatures' rule
    for (const auto& t : {std::pair<float, float>{12.f, 40.f}, {43.f, 43.f}, {15.f, 0.f}}) {
        CHECK(kept_pair_shift(t.first, t.second) == SHIFT_CONSTANT);
        CHECK(kept_pair_shift(t.first, t.second) == plan_temperatures(t.first, t.second, 70, true).shift);
    }
    for (const auto& t : {std::pair<float, float>{43.5f, 40.f}, {12.f, 200.f}, {100.f, 0.f}}) {
        CHECK(kept_pair_shift(t.first, t.second) == SHIFT_RUNNING_MAX);
        CHECK(kept_pair_shift(t.first, t.second) == plan_temperatures(t.first, t.second, 70, true).shift);
    }
    std::printf("kept_stats_plan ok\n");
    return 0;
}
