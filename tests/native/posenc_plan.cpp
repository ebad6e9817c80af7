// The launch plan of the positional encoders (range_amd/csrc/host_plan.h: posenc_plan) on the CPU, built
// with g++ under AddressSanitizer / UndefinedBehaviorSanitizer by tests/test_posenc_cpu.py: row widths for
// every kind and frequency count, every (location, frequency) covered exactly once by the tiles the
// workgroups walk, no grid dimension or LDS size out of range - also for more than 2^31 locations.
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

// the kernel's index arithmetic for work item `t` of tile `tile` (posenc_kernel.h), on the host
struct Item { int64_t b; int i; bool live; int loc_in_tile; int n_loc; };
static Item item_of(const PosencPlan& p, int F, int64_t tile, int t) {
    const int64_t k0 = tile * POSENC_BLOCK, b0 = k0 / F;
    const unsigned r0 = (unsigned)(k0 - b0 * F), u = r0 + (unsigned)t, db = u / (unsigned)F;
    return {b0 + db, (int)(u - db * (unsigned)F), k0 + t < p.items, (int)db,
            (int)((r0 + POSENC_BLOCK - 1) / (unsigned)F + 1)};
}

int main() {
    const int per_freq[PE_KINDS] = {6, 4, 6, 12, 10, 16};
    const int64_t big = (INT64_C(1) << 31) + 5;
    for (int kind = 0; kind < PE_KINDS; ++kind) {
        for (int F : {1, 16, 33, 64}) {
            for (int64_t B : {INT64_C(1), INT64_C(255), INT64_C(256), INT64_C(257), big}) {
                const PosencPlan p = posenc_plan(kind, F, B);
                CHECK(p.valid);
                CHECK(p.per_freq == per_freq[kind] && p.width == per_freq[kind] * F);
                CHECK(p.items == B * F);
                CHECK(p.block == POSENC_BLOCK && p.block % 64 == 0);
                CHECK(p.grid >= 1 && (int64_t)p.grid <= POSENC_MAX_GRID && (int64_t)p.grid <= p.n_tiles);
                CHECK((int64_t)p.grid <= std::numeric_limits<int32_t>::max());
                CHECK(p.n_tiles * POSENC_BLOCK >= p.items && (p.n_tiles - 1) * POSENC_BLOCK < p.items);
                CHECK(p.staged == (kind != PE_GRID));
                const bool single = kind == PE_SPHEREM || kind == PE_SPHEREMPLUS;
                CHECK((p.locs_per_tile > 0) == single && p.locs_per_tile <= POSENC_BLOCK);
                CHECK(p.lds_bytes == ((p.staged ? (size_t)POSENC_BLOCK * p.per_freq : 0) + 3u * p.locs_per_tile) * 8);
                CHECK(p.lds_bytes <= 64 * 1024);
                // the workgroups' grid-stride walks partition the tiles
                int64_t walked = 0;
                for (int64_t blk = 0; blk < (int64_t)p.grid; ++blk) {
                    const int64_t n = p.tiles_of(blk);
                    CHECK(n >= 1 && blk + (n - 1) * (int64_t)p.grid < p.n_tiles && blk + n * (int64_t)p.grid >= p.n_tiles);
                    walked += n;
                }
                CHECK(walked == p.n_tiles);
                CHECK(p.tiles_of(p.n_tiles) == 0);
                if (B == big) {
                    // too many items to enumerate: the first and the last tiles item by item
                    for (int64_t tile : {INT64_C(0), p.n_tiles / 2, p.n_tiles - 1})
                        for (int t = 0; t < POSENC_BLOCK; ++t) {
                            const Item it = item_of(p, F, tile, t);
                            const int64_t k = tile * POSENC_BLOCK + t;
                            CHECK(it.live == (k < p.items));
                            if (!it.live) continue;
                            CHECK(it.b == k / F && it.i == (int)(k % F) && it.b < B);
                            CHECK(it.loc_in_tile < it.n_loc && (!single || it.n_loc <= p.locs_per_tile));
                        }
                    continue;
                }
                // every (location, frequency) exactly once
                std::vector<int> seen((size_t)p.items, 0);
                for (int64_t blk = 0; blk < (int64_t)p.grid; ++blk)
                    for (int64_t tile = blk; tile < p.n_tiles; tile += p.grid)
                        for (int t = 0; t < POSENC_BLOCK; ++t) {
                            const Item it = item_of(p, F, tile, t);
                            if (!it.live) continue;
                            CHECK(it.b >= 0 && it.b < B && it.i >= 0 && it.i < F);
                            CHECK(it.loc_in_tile < it.n_loc && (!single || it.n_loc <= p.locs_per_tile));
                            seen[(size_t)(it.b * F + it.i)] += 1;
                        }
                for (int s : seen) CHECK(s == 1);
            }
        }
        // refused: F out of range, B < 1, an output beyond 2^62 bytes
        CHECK(!posenc_plan(kind, 0, 10).valid && !posenc_plan(kind, 65, 10).valid);
        CHECK(!posenc_plan(kind, 16, 0).valid && !posenc_plan(kind, 16, -3).valid);
        CHECK(!posenc_plan(kind, 64, std::numeric_limits<int64_t>::max() / 2).valid);
    }
    CHECK(!posenc_plan(-1, 16, 10).valid && !posenc_plan(PE_KINDS, 16, 10).valid);
    CHECK(posenc_per_freq(-1) == 0 && posenc_per_freq(PE_KINDS) == 0);
    // a grid smaller than the tiles: the walk takes several rounds
    {
        const PosencPlan p = posenc_plan(PE_SPHEREMPLUS, 64, big);
        CHECK((int64_t)p.grid == POSENC_MAX_GRID && p.n_tiles > (int64_t)p.grid && p.tiles_of(0) > 1);
    }
    std::printf("posenc_plan ok\n");
    return 0;
}
