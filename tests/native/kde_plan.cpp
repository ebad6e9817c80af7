// The launch plan of the KDE geo prior (range_amd/csrc/host_plan.h: kde_plan) on the CPU, built with g++ under
// AddressSanitizer / UndefinedBehaviorSanitizer by tests/test_kde_cpu.py: G by the classes with 8-byte entries, the
// query groups and the tiles of bins cover every (query, bin) pair exactly once, LDS and workspace sizes at the class
// edges (1, 8142, 16384; 16385 refused), B = 1, M = 1, forced chunks, a capped grid, the scale bits up to a total
// count of 2^31 - 1 - no row can reach 2^62 -, and the refusals.
#include <limits>

#include "plan_cover.h"

using namespace range_host;

int main() {
    const int T = NEIGHBOR_BLOCK;
    // G: the uint64 rows fit the LDS budget, one more would not (or the cap holds)
    for (int C : {1, 2, 5, 33, 2112, 2113, 4224, 4225, 8142, 8448, 8449, 16383, 16384}) {
        const int G = kde_group(C);
        CHECK(G >= 1 && G <= NEIGHBOR_MAX_GROUP && (size_t)G * C * 8 <= NEIGHBOR_COUNT_LDS);
        CHECK(G == NEIGHBOR_MAX_GROUP || (size_t)(G + 1) * C * 8 > NEIGHBOR_COUNT_LDS);
    }
    CHECK(kde_group(8142) == 2 && kde_group(33) == 8 && kde_group(16384) == 1 && kde_group(1) == 8);
    CHECK(kde_group(0) == 0 && kde_group(16385) == 0 && kde_group(-3) == 0);
    // the scale bits: the largest s <= 52 with total * 2^s < 2^62
    for (int64_t total : {INT64_C(1), INT64_C(2), INT64_C(300), INT64_C(511), INT64_C(512), INT64_C(1023), INT64_C(1024), INT64_C(1025),
                          INT64_C(436000), (INT64_C(1) << 30) - 1, INT64_C(1) << 30, KDE_MAX_TOTAL}) {
        const int s = kde_scale_bits(total);
        CHECK(s >= 31 && s <= KDE_MAX_SCALE_BITS);
        CHECK((unsigned __int128)total << s < (unsigned __int128)1 << 62);
        CHECK(s == KDE_MAX_SCALE_BITS || (unsigned __int128)total << (s + 1) >= (unsigned __int128)1 << 62);
    }
    CHECK(kde_scale_bits(1) == 52 && kde_scale_bits(1023) == 52 && kde_scale_bits(1024) == 51 && kde_scale_bits(436000) == 43);
    CHECK(kde_scale_bits(KDE_MAX_TOTAL) == 31 && kde_scale_bits(0) == 0 && kde_scale_bits(KDE_MAX_TOTAL + 1) == 0 && kde_scale_bits(-1) == 0);
    for (int C : {1, 5, 33, 8142, 16384}) {
        const int G = kde_group(C);
        for (int64_t B : {INT64_C(1), (int64_t)G - 1, (int64_t)G, (int64_t)G + 1, (int64_t)3 * G + 1, INT64_C(1000), INT64_C(24000),
                          NEIGHBOR_TARGET_WG * G - 1, NEIGHBOR_TARGET_WG * G, NEIGHBOR_TARGET_WG * G + 1, INT64_C(1) << 22}) {
            if (B < 1) continue;
            for (int64_t M : {INT64_C(1), (int64_t)T - 1, (int64_t)T, (int64_t)T + 1, INT64_C(1000), INT64_C(436000)})
                for (int chunks : {0, 1, 2, 3, 7, 64, 65, 1000})
                    for (int64_t max_grid : {INT64_C(0), INT64_C(1), INT64_C(3), INT64_C(1) << 30})
                        for (int64_t total : {M, M + 7, KDE_MAX_TOTAL}) {
                            const KdePlan p = kde_plan(B, M, C, total, max_grid, chunks);
                            CHECK(p.valid && p.block == T && p.group == G && p.vote_block == NEIGHBOR_VOTE_BLOCK);
                            CHECK(p.scale_bits == kde_scale_bits(total));
                            CHECK(p.groups == (B + G - 1) / G && p.n_tiles == (M + T - 1) / T);
                            CHECK((p.groups - 1) * p.group < B && (p.n_tiles - 1) * p.block < M);
                            const int64_t cap = max_grid ? std::min(max_grid, NEIGHBOR_MAX_GRID) : NEIGHBOR_MAX_GRID;
                            CHECK(p.grid >= 1 && (int64_t)p.grid <= cap && (int64_t)p.grid <= p.groups);
                            CHECK(p.select_grid >= 1 && (int64_t)p.select_grid <= cap && (int64_t)p.select_grid <= B);
                            CHECK(p.chunks >= 1 && p.chunks <= NEIGHBOR_MAX_CHUNKS && p.chunks <= p.n_tiles && (int64_t)p.chunks <= cap);
                            if (chunks > 0) CHECK(p.chunks <= chunks);
                            if (chunks == 0 && p.groups >= NEIGHBOR_TARGET_WG) CHECK(p.chunks == 1);
                            // uint64 rows, 16-byte aligned, then the queries' parameters: inside the CU's 160 KB
                            CHECK(p.lds_bytes >= (size_t)G * C * 8 + (size_t)G * NEIGHBOR_QUERY_LDS && p.lds_bytes <= 160 * 1024);
                            CHECK(((p.lds_bytes - (size_t)G * NEIGHBOR_QUERY_LDS) % 16) == 0);
                            // the kernel's own offset of the parameters (neighbor_query_offset): the rows rounded up to 16 bytes, two words
                            CHECK((size_t)(((int64_t)G * C + 1) & ~INT64_C(1)) * 8 + (size_t)G * NEIGHBOR_QUERY_LDS == p.lds_bytes);
                            if (p.chunks == 1) {
                                CHECK(p.ws_ints == 0 && p.ws_bytes == 0 && p.fold_grid == 0);
                            } else {
                                CHECK(p.ws_ints == (size_t)p.chunks * p.groups * G * C && p.ws_bytes == p.ws_ints * 8);
                                CHECK(p.ws_bytes <= NEIGHBOR_MAX_WS);
                                CHECK(p.fold_grid >= 1 && (int64_t)p.fold_grid <= cap && (int64_t)p.fold_grid <= p.groups);
                                // the last partial sum a workgroup writes
                                CHECK(((size_t)(p.chunks - 1) * p.groups + (p.groups - 1)) * G * C + (size_t)G * C - 1 < p.ws_ints);
                            }
                            if (total == M && check_cover(p, B, M)) return 1;
                        }
        }
    }
    // the design shapes: 24 000 queries, 8142 classes - 12 000 groups of 2, no split; a 128 KB row at the class cap
    {
        const KdePlan p = kde_plan(24000, 436000, 8142, 436000);
        CHECK(p.valid && p.group == 2 && p.groups == 12000 && p.chunks == 1 && p.ws_bytes == 0 && p.n_tiles == 1704 && p.scale_bits == 43);
        const KdePlan s = kde_plan(8, 436000, 8142, 436000);
        CHECK(s.valid && s.groups == 4 && s.chunks == NEIGHBOR_MAX_CHUNKS && s.ws_bytes == (size_t)64 * 4 * 2 * 8142 * 8);
        const KdePlan c = kde_plan(1, 1, KDE_MAX_CLASSES, 1);
        CHECK(c.valid && c.group == 1 && c.lds_bytes == (size_t)128 * 1024 + NEIGHBOR_QUERY_LDS && c.scale_bits == 52 && c.chunks == 1);
    }
    // refused
    CHECK(!kde_plan(0, 5, 3, 5).valid && !kde_plan(5, 0, 3, 5).valid && !kde_plan(-1, 5, 3, 5).valid);
    CHECK(!kde_plan(5, 5, 0, 5).valid && !kde_plan(5, 5, KDE_MAX_CLASSES + 1, 5).valid && kde_plan(5, 5, KDE_MAX_CLASSES, 5).valid);
    CHECK(!kde_plan(5, 5, 3, 4).valid && !kde_plan(5, 5, 3, KDE_MAX_TOTAL + 1).valid && !kde_plan(5, 5, 3, -1).valid);
    CHECK(!kde_plan(5, 5, 3, 5, -1, 0).valid && !kde_plan(5, 5, 3, 5, 0, -1).valid);
    CHECK(!kde_plan(NEIGHBOR_MAX_QUERIES + 1, 5, 3, 5).valid && !kde_plan(5, NEIGHBOR_MAX_POINTS + 1, 3, KDE_MAX_TOTAL).valid);
    CHECK(!kde_plan(std::numeric_limits<int64_t>::max(), 5, 3, 5).valid);
    CHECK(kde_plan(NEIGHBOR_MAX_QUERIES, NEIGHBOR_MAX_POINTS, KDE_MAX_CLASSES, KDE_MAX_TOTAL).valid);
    // the neighbour plan did not move with the shared geometry
    {
        const NeighborPlan n = neighbor_plan(24000, 436000, 8142, 1500);
        CHECK(n.valid && n.group == 4 && n.groups == 6000 && n.chunks == 1 && n.lds_bytes == (size_t)4 * 8142 * 4 + 4 * NEIGHBOR_QUERY_LDS);
    }
    std::printf("kde_plan ok classes=%d bits=%d\n", KDE_MAX_CLASSES, KDE_MAX_SCALE_BITS);
    return 0;
}
