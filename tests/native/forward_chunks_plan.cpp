// The chunk plan of the overlapped forward (range_amd/csrc/host_plan.h: plan_forward_chunks) on the CPU, built
// with g++ under AddressSanitizer / UndefinedBehaviorSanitizer by tests/test_forward_overlap_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <vector>

#include "../../range_amd/csrc/host_plan.h"

using namespace range_host;

#define CHECK(cond)                                                                                            \
    do {                                                                                                       \
        if (!(cond)) {                                                                                         \
            std::printf("FAILED line %d: %s (n_cu %d rows %lld B %lld)\n", __LINE__, #cond, n_cu, (long long)n_rows, \
                        (long long)B);                                                                         \
            return 1;                                                                                          \
        }                                                                                                      \
    } while (0)

int main() {
    // (engine_prims.h / pass1.h: QTILE, BLK, VAL_DIM, MAX_TOPK, P1_WG_PER_CU, ...)
    const PlanConsts K{64, 16, 1024, 16, 4, 32, 8, 128, 2, 64};
    long long planned = 0;
    for (int n_cu : {256, 304, 64})
        for (int64_t n_rows : {4100, 50016, 100000, 1000000}) {
            for (int64_t B = 1; B <= 40000; ++B) {
                const Pass1Plan p1 = plan_pass1(n_cu, n_rows, B, false, 0, K);
                for (int streamk = 0; streamk < 2; ++streamk) {
                    const Pass2Plan p2 = plan_pass2(n_cu, n_rows, B, streamk != 0, K);
                    const int T = p2.n_qtiles, ns = p2.n_splits;
                    // the switch off, the stream-K walk, a single tile: no plan
                    CHECK(plan_forward_chunks(n_cu, p1, p2, 0).tiles.empty());
                    const FwdChunkPlan p = plan_forward_chunks(n_cu, p1, p2, -1);
                    if (p2.streamk || T < 2) {
                        CHECK(p.tiles.empty());
                        CHECK(plan_forward_chunks(n_cu, p1, p2, 1).tiles.empty());
                    }
                    if (p2.streamk) continue;
                    // forced chunks: n tiles each, the last one the rest; one chunk is no plan
                    for (int n : {1, 2, 8}) {
                        const FwdChunkPlan f = plan_forward_chunks(n_cu, p1, p2, n);
                        if (T <= n) { CHECK(f.tiles.empty()); continue; }
                        CHECK((int)f.tiles.size() == (T + n - 1) / n && f.p1_splits == p1.n_splits && f.p2_splits == ns);
                        int sum = 0;
                        for (size_t i = 0; i < f.tiles.size(); ++i) {
                            CHECK(f.tiles[i] == (i + 1 < f.tiles.size() ? n : T - sum));
                            sum += f.tiles[i];
                        }
                        CHECK(sum == T && f.tiles.back() >= 1);
                    }
                    if (p.tiles.empty()) continue;
                    ++planned;
                    // the rule's plan: at least two chunks that cover the tiles once, in order; every chunk whole
                    // rounds of pass 2 at least 98 % full; no round more than the single launch has; the
                    // smallest chunk first; the whole batch's split counts
                    CHECK(p.tiles.size() >= 2 && p.p1_splits == p1.n_splits && p.p2_splits == ns);
                    const int64_t rounds_all = ((int64_t)T * ns + n_cu - 1) / n_cu;
                    int64_t sum = 0, rounds = 0;
                    for (int t : p.tiles) {
                        CHECK(t >= 1 && t >= p.tiles[0]);
                        const int64_t r = ((int64_t)t * ns + n_cu - 1) / n_cu;
                        CHECK((int64_t)t * ns * 100 >= 98 * r * n_cu);
                        sum += t;
                        rounds += r;
                    }
                    CHECK(sum == T && rounds == rounds_all);
                }
            }
        }
    {
        // the benchmark: 10 000 queries against 100 000 rows on 256 CUs - 157 tiles x 13 splits in 8 rounds
        const int n_cu = 256;
        const int64_t n_rows = 100000, B = 10000;
        const Pass1Plan p1 = plan_pass1(n_cu, n_rows, B, false, 0, K);
        const Pass2Plan p2 = plan_pass2(n_cu, n_rows, B, true, K);
        CHECK(p2.n_qtiles == 157 && p2.n_splits == 13 && !p2.streamk);
        const FwdChunkPlan p = plan_forward_chunks(n_cu, p1, p2, -1);
        CHECK((p.tiles == std::vector<int>{39, 59, 59}));
        CHECK(planned > 0);
    }
    std::printf("forward_chunks_plan ok (%lld planned shapes)\n", planned);
    return 0;
}
