// The launch plan of the embedding map (range_amd/csrc/host_plan.h: map_plan) on the CPU, built with g++ under
// AddressSanitizer / UndefinedBehaviorSanitizer by tests/test_icamap_cpu.py: the slabs of the ICA step cover every
// row exactly once and do not depend on the grid, the walks of a capped grid reach every slab / row group / block,
// grids, slab counts and workspace sizes are in range - also for 2^40 rows - and the refusals.
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

// the kernels' walks (map_kernels.h) on the host
static int check_cover(const MapPlan& p, int64_t n) {
    // ICA step: workgroup x computes slabs x, x + grid, ...; thread t of slab s takes rows s*chunk + j*block + t
    int64_t slabs = 0, rows = 0;
    for (int64_t x = 0; x < (int64_t)p.step_grid; ++x) {
        const int64_t k = p.slabs_of(x);
        CHECK(k >= 1 && x + (k - 1) * (int64_t)p.step_grid < p.slabs && x + k * (int64_t)p.step_grid >= p.slabs);
        slabs += k;
    }
    CHECK(slabs == p.slabs && p.slabs_of(p.slabs) == 0);
    for (int64_t s = 0; s < p.slabs; ++s) {
        const int64_t r = p.slab_rows(s, n);
        CHECK(r >= 1 && r <= p.chunk);                 // no slab is empty: every slab of the workspace is written
        rows += r;
    }
    CHECK(rows == n && p.slab_rows(p.slabs, n) == 0);
    if (n <= (1 << 17)) {
        std::vector<int> seen((size_t)n, 0);
        for (int64_t x = 0; x < (int64_t)p.step_grid; ++x)
            for (int64_t s = x; s < p.slabs; s += p.step_grid)
                for (int64_t j = 0; j < p.ipt; ++j)
                    for (int t = 0; t < p.block; ++t) {
                        const int64_t i = s * p.ipt * p.block + j * p.block + t;
                        if (i < n) seen[(size_t)i] += 1;
                    }
        for (int v : seen) CHECK(v == 1);
        // projection: row groups of MAP_PROJ_ROWS, equalisation: blocks of MAP_BLOCK, both grid-stride
        std::vector<int> pr((size_t)n, 0), eq((size_t)n, 0);
        for (int64_t x = 0; x < (int64_t)p.proj_grid; ++x)
            for (int64_t g = x; g < p.proj_groups; g += p.proj_grid)
                for (int r = 0; r < MAP_PROJ_ROWS; ++r)
                    if (g * MAP_PROJ_ROWS + r < n) pr[(size_t)(g * MAP_PROJ_ROWS + r)] += 1;
        for (int64_t i0 = 0; i0 < (int64_t)p.eq_grid * p.block; ++i0)
            for (int64_t i = i0; i < n; i += (int64_t)p.eq_grid * p.block) eq[(size_t)i] += 1;
        for (int v : pr) CHECK(v == 1);
        for (int v : eq) CHECK(v == 1);
    }
    return 0;
}

int main() {
    const int64_t big = INT64_C(1) << 40;
    const int64_t share = (int64_t)MAP_BLOCK * MAP_MIN_IPT;
    for (int64_t n : {INT64_C(1), INT64_C(63), INT64_C(64), INT64_C(65), INT64_C(255), INT64_C(256), INT64_C(257), share - 1,
                      share, share + 1, 3 * share + 1, INT64_C(1000000), MAP_MAX_SLABS * share + 1, INT64_C(1) << 33, big})
        for (int c : {1, 2, 3, 5, 8})
            for (int64_t max_grid : {INT64_C(0), INT64_C(1), INT64_C(3), INT64_C(7), INT64_C(100000)}) {
                const MapPlan p = map_plan(n, c, max_grid);
                CHECK(p.valid && p.block == MAP_BLOCK && p.block % 64 == 0);
                CHECK(p.ipt >= MAP_MIN_IPT && p.chunk == p.ipt * p.block);
                CHECK(p.slabs == (n + p.chunk - 1) / p.chunk && p.slabs >= 1 && p.slabs <= MAP_MAX_SLABS);
                CHECK(p.slab_doubles == c * c + c);
                CHECK(p.ws_bytes == (size_t)p.slabs * (size_t)(c * c + c) * 8 && p.ws_bytes <= MAP_MAX_SLABS * 72 * 8);
                CHECK(p.proj_groups == (n + MAP_PROJ_ROWS - 1) / MAP_PROJ_ROWS && p.eq_blocks == (n + p.block - 1) / p.block);
                for (unsigned g : {p.step_grid, p.proj_grid, p.eq_grid}) {
                    CHECK(g >= 1 && (int64_t)g <= MAP_MAX_GRID);
                    if (max_grid > 0) CHECK((int64_t)g <= max_grid);
                }
                CHECK((int64_t)p.step_grid <= p.slabs && (int64_t)p.proj_grid <= p.proj_groups && (int64_t)p.eq_grid <= p.eq_blocks);
                // the cut of the rows into slabs is the grid's business nowhere
                const MapPlan q = map_plan(n, c, 0);
                CHECK(q.ipt == p.ipt && q.chunk == p.chunk && q.slabs == p.slabs && q.ws_bytes == p.ws_bytes);
                // the last row a thread of the last slab may index stays below 2^63
                CHECK(p.slabs * p.chunk >= n && (p.slabs - 1) * p.chunk < n);
                if (check_cover(p, n)) return 1;
            }
    // the design shape: 10^6 rows in 977 slabs of 1024 rows, 12 doubles each for three components
    {
        const MapPlan p = map_plan(1000000, 3, 0);
        CHECK(p.ipt == 4 && p.chunk == 1024 && p.slabs == 977 && p.step_grid == 977 && p.ws_bytes == 977u * 12 * 8);
        CHECK(p.proj_grid == MAP_MAX_GRID && p.eq_grid == MAP_MAX_GRID);
    }
    // one row beyond a full capped grid: some workgroup makes a second trip
    {
        const MapPlan p = map_plan(3 * share + 1, 3, 3);
        CHECK(p.slabs == 4 && p.step_grid == 3 && p.slabs_of(0) == 2 && p.slabs_of(1) == 1 && p.slab_rows(3, 3 * share + 1) == 1);
    }
    // refused
    CHECK(!map_plan(0, 3, 0).valid && !map_plan(-5, 3, 0).valid && !map_plan(big + 1, 3, 0).valid);
    CHECK(!map_plan(std::numeric_limits<int64_t>::max(), 3, 0).valid);
    CHECK(!map_plan(100, 0, 0).valid && !map_plan(100, MAP_MAX_C + 1, 0).valid && !map_plan(100, -1, 0).valid);
    CHECK(!map_plan(100, 3, -1).valid);
    CHECK(map_plan(big, MAP_MAX_C, 0).valid);
    std::printf("map_plan ok block=%d share=%lld max_slabs=%lld\n", MAP_BLOCK, (long long)share, (long long)MAP_MAX_SLABS);
    return 0;
}
