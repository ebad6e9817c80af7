// The launch plan of the neighbour / grid geo priors (range_amd/csrc/host_plan.h: neighbor_plan) on the CPU, built
// with g++ under AddressSanitizer / UndefinedBehaviorSanitizer by tests/test_neighbors_cpu.py: the query groups the
// workgroups walk and the training tiles the chunks walk cover every (query, point) pair exactly once, LDS and
// workspace sizes are in range at and around every tile, group and cap edge, the selection's digits cover the 64
// bits of a key exactly once, and the refusals.
#include <limits>

#include "plan_cover.h"

using namespace range_host;

int main() {
    const int T = NEIGHBOR_BLOCK;
    // the selection's digits: every bit of the key in exactly one pass, top down
    {
        uint64_t covered = 0;
        int last = 64;
        for (int pass = 0; pass < NEIGHBOR_PASSES; ++pass) {
            const int shift = NeighborPlan::shift_of(pass);
            CHECK(shift >= 0 && shift < 64 && shift < last);
            const int width = last - shift;
            CHECK(width >= 1 && width <= NEIGHBOR_DIGIT_BITS);
            for (int b = shift; b < last; ++b) {
                CHECK(!(covered >> b & 1));
                covered |= UINT64_C(1) << b;
            }
            // the largest digit of the pass indexes the histogram
            CHECK(((~UINT64_C(0) >> shift) & (uint64_t)(NEIGHBOR_BINS - 1)) < (uint64_t)NEIGHBOR_BINS);
            if (pass == 0) CHECK((~UINT64_C(0) >> shift) < (uint64_t)NEIGHBOR_BINS);
            last = shift;
        }
        CHECK(covered == ~UINT64_C(0) && last == 0 && NEIGHBOR_BINS % NEIGHBOR_BLOCK == 0);
    }
    // G by the classes: the rows fit the LDS budget, one more would not (or the cap holds)
    for (int C : {1, 2, 5, 33, 4223, 4224, 4225, 8142, 8448, 8449, 11264, 11265, 16896, 16897, 32767, 32768}) {
        const int G = neighbor_group(C);
        CHECK(G >= 1 && G <= NEIGHBOR_MAX_GROUP && (size_t)G * C * 4 <= NEIGHBOR_COUNT_LDS);
        CHECK(G == NEIGHBOR_MAX_GROUP || (size_t)(G + 1) * C * 4 > NEIGHBOR_COUNT_LDS);
    }
    CHECK(neighbor_group(8142) == 4 && neighbor_group(33) == 8 && neighbor_group(32768) == 1);
    CHECK(neighbor_group(0) == 0 && neighbor_group(32769) == 0 && neighbor_group(-3) == 0);
    for (int C : {1, 5, 33, 8142, 32768}) {
        const int G = neighbor_group(C);
        for (int64_t B : {INT64_C(1), (int64_t)G - 1, (int64_t)G, (int64_t)G + 1, (int64_t)3 * G + 1, INT64_C(1000), INT64_C(24000),
                          NEIGHBOR_TARGET_WG * G - 1, NEIGHBOR_TARGET_WG * G, NEIGHBOR_TARGET_WG * G + 1, INT64_C(1) << 22}) {
            if (B < 1) continue;
            for (int64_t N : {INT64_C(1), (int64_t)T - 1, (int64_t)T, (int64_t)T + 1, INT64_C(1000), INT64_C(436000)})
                for (int chunks : {0, 1, 2, 3, 7, 64, 65, 1000})
                    for (int64_t max_grid : {INT64_C(0), INT64_C(1), INT64_C(3), INT64_C(1) << 30}) {
                        for (int64_t k : {INT64_C(0), INT64_C(1), N}) {
                            const NeighborPlan p = neighbor_plan(B, N, C, k, max_grid, chunks);
                            CHECK(p.valid && p.block == T && p.block % 64 == 0 && p.group == G);
                            CHECK(p.vote_block == NEIGHBOR_VOTE_BLOCK && p.vote_block % p.block == 0 && p.vote_block <= 1024);
                            CHECK(p.groups == (B + G - 1) / G && p.n_tiles == (N + T - 1) / T);
                            const int64_t cap = max_grid ? std::min(max_grid, NEIGHBOR_MAX_GRID) : NEIGHBOR_MAX_GRID;
                            CHECK(p.grid >= 1 && (int64_t)p.grid <= cap && (int64_t)p.grid <= p.groups);
                            CHECK(p.select_grid >= 1 && (int64_t)p.select_grid <= cap && (int64_t)p.select_grid <= B);
                            CHECK(p.chunks >= 1 && p.chunks <= NEIGHBOR_MAX_CHUNKS && p.chunks <= p.n_tiles && (int64_t)p.chunks <= cap);
                            if (chunks > 0) CHECK(p.chunks <= chunks);
                            if (chunks == 0 && p.groups >= NEIGHBOR_TARGET_WG) CHECK(p.chunks == 1);
                            // count rows, 16-byte aligned, then the queries' parameters: inside the CU's 160 KB
                            CHECK(p.lds_bytes >= (size_t)G * C * 4 + (size_t)G * NEIGHBOR_QUERY_LDS && p.lds_bytes <= 160 * 1024);
                            CHECK(((p.lds_bytes - (size_t)G * NEIGHBOR_QUERY_LDS) % 16) == 0);
                            CHECK(p.select_lds <= 64 * 1024);
                            if (p.chunks == 1) {
                                CHECK(p.ws_ints == 0 && p.ws_bytes == 0 && p.fold_grid == 0);
                            } else {
                                CHECK(p.ws_ints == (size_t)p.chunks * p.groups * G * C && p.ws_bytes == p.ws_ints * 4);
                                CHECK(p.ws_bytes <= NEIGHBOR_MAX_WS);
                                CHECK(p.fold_grid >= 1 && (int64_t)p.fold_grid <= cap && (int64_t)p.fold_grid <= p.groups);
                                // the last partial count a workgroup writes
                                CHECK(((size_t)(p.chunks - 1) * p.groups + (p.groups - 1)) * G * C + (size_t)G * C - 1 < p.ws_ints);
                            }
                            if (k == 0 && check_cover(p, B, N)) return 1;
                        }
                    }
        }
    }
    // the design shape: 24 000 queries, 436 000 points, 8142 classes - 6000 groups of 4, no split
    {
        const NeighborPlan p = neighbor_plan(24000, 436000, 8142, 1500);
        CHECK(p.valid && p.group == 4 && p.groups == 6000 && p.chunks == 1 && p.ws_bytes == 0 && p.n_tiles == 1704);
        const NeighborPlan s = neighbor_plan(8, 436000, 8142, 0);
        CHECK(s.valid && s.groups == 2 && s.chunks == NEIGHBOR_MAX_CHUNKS && s.ws_bytes == (size_t)64 * 2 * 4 * 8142 * 4);
    }
    // refused
    CHECK(!neighbor_plan(0, 5, 3, 0).valid && !neighbor_plan(5, 0, 3, 0).valid && !neighbor_plan(-1, 5, 3, 0).valid);
    CHECK(!neighbor_plan(5, 5, 0, 0).valid && !neighbor_plan(5, 5, NEIGHBOR_MAX_CLASSES + 1, 0).valid);
    CHECK(neighbor_plan(5, 5, NEIGHBOR_MAX_CLASSES, 5).valid);
    CHECK(!neighbor_plan(5, 5, 3, 6).valid && !neighbor_plan(5, 5, 3, -1).valid);
    CHECK(!neighbor_plan(5, 5, 3, 0, -1, 0).valid && !neighbor_plan(5, 5, 3, 0, 0, -1).valid);
    CHECK(!neighbor_plan(NEIGHBOR_MAX_QUERIES + 1, 5, 3, 0).valid && !neighbor_plan(5, NEIGHBOR_MAX_POINTS + 1, 3, 0).valid);
    CHECK(!neighbor_plan(std::numeric_limits<int64_t>::max(), 5, 3, 0).valid);
    CHECK(neighbor_plan(NEIGHBOR_MAX_QUERIES, NEIGHBOR_MAX_POINTS, NEIGHBOR_MAX_CLASSES, NEIGHBOR_MAX_POINTS).valid);
    std::printf("neighbor_plan ok block=%d passes=%d\n", NEIGHBOR_BLOCK, NEIGHBOR_PASSES);
    return 0;
}
