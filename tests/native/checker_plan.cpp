// The launch plan of the checkerboard task's nearest-support scan (range_amd/csrc/host_plan.h: checker_plan) on
// the CPU, built with g++ under AddressSanitizer / UndefinedBehaviorSanitizer by tests/test_checker_cpu.py:
// the query blocks the workgroups walk and the support tiles the chunks walk cover every (query, support)
// pair exactly once, grids and workspace sizes are in range - also for 2^33 queries - and the refusals.
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../range_amd/csrc/host_plan.h"

using namespace range_host;

#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);             \
            return 1;                                                         \
        }                                                                     \
    } while (0)

// the kernel's walk (checker_kernel.h) on the host: how often query i / support j is visited
static int check_cover(const CheckerPlan& p, int64_t Q, int64_t S) {
    const bool big_q = Q > (1 << 20);
    std::vector<int> q_seen(big_q ? 0 : (size_t)Q, 0), s_seen((size_t)S, 0);
    int64_t blocks = 0;
    for (int64_t x = 0; x < (int64_t)p.grid_x; ++x) {
        const int64_t n = p.blocks_of(x);
        CHECK(n >= 1 && x + (n - 1) * (int64_t)p.grid_x < p.q_blocks && x + n * (int64_t)p.grid_x >= p.q_blocks);
        blocks += n;
        if (big_q) continue;
        for (int64_t qb = x; qb < p.q_blocks; qb += p.grid_x)
            for (int t = 0; t < p.block; ++t) {
                const int64_t i = qb * p.block + t;
                if (i < Q) q_seen[(size_t)i] += 1;
            }
    }
    CHECK(blocks == p.q_blocks && p.blocks_of(p.q_blocks) == 0);
    for (int v : q_seen) CHECK(v == 1);
    if (big_q) {
        // the first and the last block by hand
        CHECK((p.q_blocks - 1) * p.block < Q && p.q_blocks * p.block >= Q);
    }
    int64_t tiles = 0;
    for (int y = 0; y < p.chunks; ++y) {
        const int64_t n = p.tiles_of(y);
        CHECK(n >= 1);                      // no chunk is empty: every partial pair of the workspace is written
        tiles += n;
        for (int64_t tile = y; tile < p.s_tiles; tile += p.chunks) {
            const int64_t j0 = tile * p.tile;
            const int64_t cnt = S - j0 < p.tile ? S - j0 : p.tile;
            CHECK(cnt >= 1 && cnt <= p.tile);
            for (int64_t k = 0; k < cnt; ++k) s_seen[(size_t)(j0 + k)] += 1;
        }
    }
    CHECK(tiles == p.s_tiles && p.tiles_of(p.s_tiles) == 0);
    for (int v : s_seen) CHECK(v == 1);
    return 0;
}

int main() {
    const int T = CHECKER_TILE;
    const int64_t big = INT64_C(1) << 33;
    for (int64_t Q : {INT64_C(1), INT64_C(63), INT64_C(64), INT64_C(65), INT64_C(257), INT64_C(10000), big})
        for (int64_t S : {INT64_C(1), (int64_t)T - 1, (int64_t)T, (int64_t)T + 1, (int64_t)2 * T + 1, INT64_C(100000)})
            for (int max_chunks : {0, 1, 2, 3, 7, 1000}) {
                const CheckerPlan p = checker_plan(Q, S, false, max_chunks);
                CHECK(p.valid);
                CHECK(p.tile == T && p.block == CHECKER_BLOCK && p.block % 64 == 0);
                CHECK(p.q_blocks == (Q + p.block - 1) / p.block && p.s_tiles == (S + T - 1) / T);
                CHECK(p.grid_x >= 1 && (int64_t)p.grid_x <= CHECKER_MAX_GRID && (int64_t)p.grid_x <= p.q_blocks);
                CHECK(p.chunks >= 1 && p.chunks <= CHECKER_MAX_CHUNKS && p.chunks <= p.s_tiles && p.chunks <= 65535);
                if (max_chunks > 0) CHECK(p.chunks <= max_chunks);
                if (max_chunks > 0 && max_chunks <= CHECKER_MAX_CHUNKS) CHECK(p.chunks == (int)std::min<int64_t>(max_chunks, p.s_tiles));
                if (max_chunks == 0) {
                    // a small Q is spread over the chip as far as the tiles allow; a large one is not split
                    if (p.q_blocks >= CHECKER_TARGET_WG) CHECK(p.chunks == 1);
                    else CHECK(p.chunks == CHECKER_MAX_CHUNKS || p.chunks == p.s_tiles ||
                               p.q_blocks * p.chunks >= CHECKER_TARGET_WG);
                }
                CHECK(p.lds_bytes == (size_t)3 * T * 8 && p.lds_bytes <= 64 * 1024);
                if (p.chunks == 1) {
                    CHECK(p.ws_pairs == 0 && p.ws_bytes == 0 && p.merge_grid == 0);
                } else {
                    CHECK(p.ws_pairs == (size_t)p.chunks * (size_t)Q && p.ws_bytes == p.ws_pairs * 16);
                    CHECK(p.merge_grid >= 1 && (int64_t)p.merge_grid <= CHECKER_MAX_GRID);
                    // the last partial pair a workgroup writes: (chunks - 1) * Q + (Q - 1)
                    CHECK((size_t)(p.chunks - 1) * (size_t)Q + (size_t)(Q - 1) < p.ws_pairs);
                }
                if (check_cover(p, Q, S)) return 1;
            }
    // the design shapes
    CHECK(checker_plan(10000, 200, false, 0).chunks == 1);
    CHECK(checker_plan(10000, 10000, false, 0).chunks == 40);
    CHECK(checker_plan(1000000, 10000, false, 0).chunks == 1);
    // exclude_self needs the same points on both sides, at least two
    CHECK(checker_plan(200, 200, true, 0).valid && checker_plan(2, 2, true, 0).valid);
    CHECK(!checker_plan(200, 201, true, 0).valid && !checker_plan(1, 1, true, 0).valid);
    // refused
    CHECK(!checker_plan(0, 5, false, 0).valid && !checker_plan(5, 0, false, 0).valid);
    CHECK(!checker_plan(-1, 5, false, 0).valid && !checker_plan(5, -7, false, 0).valid);
    CHECK(!checker_plan(5, 5, false, -1).valid);
    CHECK(!checker_plan(CHECKER_MAX_POINTS + 1, 5, false, 0).valid && !checker_plan(5, CHECKER_MAX_POINTS + 1, false, 0).valid);
    CHECK(!checker_plan(std::numeric_limits<int64_t>::max(), 5, false, 0).valid);
    CHECK(checker_plan(CHECKER_MAX_POINTS, CHECKER_MAX_POINTS, false, 0).valid);
    std::printf("checker_plan ok tile=%d block=%d\n", CHECKER_TILE, CHECKER_BLOCK);
    return 0;
}
