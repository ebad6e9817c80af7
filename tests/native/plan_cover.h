// What the native plan programs of the geo priors share (neighbor_plan.cpp, kde_plan.cpp): CHECK and the scan's
// walk (neighbor_kernel.h: neighbor_vote_body) on the host.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../range_amd/csrc/host_plan.h"

#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);             \
            return 1;                                                         \
        }                                                                     \
    } while (0)

// how often query i / training point (bin) j is visited: exactly once each
static int check_cover(const range_host::NeighborPlan& p, int64_t B, int64_t N) {
    if (B <= (1 << 16)) {
        std::vector<int> seen((size_t)B, 0);
        int64_t groups = 0;
        for (int64_t x = 0; x < (int64_t)p.grid; ++x) {
            CHECK(p.groups_of(x) >= 1);
            groups += p.groups_of(x);
            for (int64_t grp = x; grp < p.groups; grp += p.grid)
                for (int g = 0; g < p.group; ++g)
                    if (grp * p.group + g < B) seen[(size_t)(grp * p.group + g)] += 1;
        }
        CHECK(groups == p.groups && p.groups_of(p.groups) == 0);
        for (int v : seen) CHECK(v == 1);
    }
    CHECK((p.groups - 1) * p.group < B && p.groups * p.group >= B);
    if (N <= (1 << 20)) {
        std::vector<int> seen((size_t)N, 0);
        int64_t tiles = 0;
        for (int y = 0; y < p.chunks; ++y) {
            CHECK(p.tiles_of(y) >= 1);          // no chunk is empty: every partial row of the workspace is written
            tiles += p.tiles_of(y);
            for (int64_t tile = y; tile < p.n_tiles; tile += p.chunks)
                for (int t = 0; t < p.block; ++t)
                    if (tile * p.block + t < N) seen[(size_t)(tile * p.block + t)] += 1;
        }
        CHECK(tiles == p.n_tiles && p.tiles_of(p.n_tiles) == 0);
        for (int v : seen) CHECK(v == 1);
    }
    CHECK((p.n_tiles - 1) * p.block < N && p.n_tiles * p.block >= N);
    return 0;
}
