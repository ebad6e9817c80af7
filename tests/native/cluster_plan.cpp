// The launch plan and the cut of the cluster map (range_amd/csrc/host_plan.h: cluster_plan, cluster_tile_of,
// cluster_cut) on the CPU, built with g++ under AddressSanitizer / UndefinedBehaviorSanitizer by
// tests/test_cluster_cpu.py: every walk of the kernels covers every row / tile / item exactly once under any grid
// cap, the workspace regions do not overlap, sizes do not overflow at 2^17 rows, the refusals; the cut on hand-made
// merge lists, equal heights and k = 1 and k = n among them.
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

// the kernels' walks (cluster_kernels.h) on the host
static int check_cover(const ClusterPlan& p, int64_t n) {
    // normaliser: workgroup x takes row groups x, x + grid, ...; wave w of a group its row w
    std::vector<int> seen((size_t)n, 0);
    for (int64_t x = 0; x < (int64_t)p.norm_grid; ++x)
        for (int64_t g = x; g < p.norm_groups; g += p.norm_grid)
            for (int w = 0; w < CLUSTER_NORM_ROWS; ++w)
                if (g * CLUSTER_NORM_ROWS + w < n) seen[(size_t)(g * CLUSTER_NORM_ROWS + w)] += 1;
    for (int v : seen) CHECK(v == 1);
    // the list kernels: thread t owns rows [t * serial_rows, (t + 1) * serial_rows), ascending over the threads
    std::fill(seen.begin(), seen.end(), 0);
    int64_t last = -1;
    for (int t = 0; t < p.serial_block; ++t) {
        const int64_t lo = std::min(n, (int64_t)t * p.serial_rows), hi = std::min(n, lo + p.serial_rows);
        for (int64_t r = lo; r < hi; ++r) {
            CHECK(r == last + 1);
            last = r;
            seen[(size_t)r] += 1;
        }
    }
    for (int v : seen) CHECK(v == 1);
    CHECK(p.serial_rows * p.serial_block >= n && p.serial_rows * p.serial_block < (INT64_C(1) << 31));
    // the scan: workgroup x takes list entries x, x + grid, ... of up to n stale rows
    std::fill(seen.begin(), seen.end(), 0);
    for (int64_t active : {n, n / 2 + 1, INT64_C(2)}) {
        const int64_t grid = p.grid_of(active);
        CHECK(grid >= 1 && grid <= p.cap && grid <= std::max<int64_t>(active, 1));
        int64_t items = 0;
        for (int64_t x = 0; x < grid; ++x) items += p.items_of(x, active, grid);
        CHECK(items == active);
    }
    // merges: items (pair, chunk): every column of every pair's row once
    CHECK(p.chunks == (n + CLUSTER_CHUNK - 1) / CLUSTER_CHUNK && p.chunks * CLUSTER_CHUNK >= n);
    for (int64_t pairs : {INT64_C(1), INT64_C(3), n / 2}) {
        if (pairs < 1) continue;
        const int64_t items = pairs * p.chunks, grid = p.grid_of(items);
        CHECK(items < (INT64_C(1) << 31) && grid >= 1 && grid <= p.cap);
        if (n <= 1024) {
            std::vector<int> cols((size_t)(pairs * n), 0);
            for (int64_t x = 0; x < grid; ++x)
                for (int64_t it = x; it < items; it += grid) {
                    const int64_t t = it / p.chunks, c = it % p.chunks;
                    const int64_t k1 = std::min(n, (c + 1) * CLUSTER_CHUNK);
                    for (int64_t th = 0; th < p.block; ++th)
                        for (int64_t k = c * CLUSTER_CHUNK + th; k < k1; k += p.block) cols[(size_t)(t * n + k)] += 1;
                }
            for (int v : cols) CHECK(v == 1);
        }
    }
    // the distance finish: the tile triangle, every entry of the matrix written once
    CHECK(p.tiles == (n + CLUSTER_TILE - 1) / CLUSTER_TILE && p.fin_items == p.tiles * (p.tiles + 1) / 2);
    int64_t t = 0;
    const int64_t step = p.fin_items > 200000 ? 997 : 1;      // (every tile for the small shapes, a stride beyond)
    for (int64_t ti = 0; ti < p.tiles; ++ti)
        for (int64_t tj = 0; tj <= ti; ++tj, ++t) {
            if (t % step && t != p.fin_items - 1) continue;
            int64_t a, b;
            cluster_tile_of(t, a, b);
            CHECK(a == ti && b == tj);
        }
    CHECK(t == p.fin_items);
    if (n <= 300) {
        std::vector<int> ent((size_t)(n * n), 0);
        for (int64_t x = 0; x < (int64_t)p.fin_grid; ++x)
            for (int64_t it = x; it < p.fin_items; it += p.fin_grid) {
                int64_t ti, tj;
                cluster_tile_of(it, ti, tj);
                for (int r = 0; r < CLUSTER_TILE; ++r)
                    for (int c = 0; c < CLUSTER_TILE; ++c) {
                        const int64_t i = ti * CLUSTER_TILE + r, j = tj * CLUSTER_TILE + c;
                        if (ti != tj) {
                            if (i < n && j < n) ent[(size_t)(i * n + j)] += 1;
                            const int64_t i2 = tj * CLUSTER_TILE + r, j2 = ti * CLUSTER_TILE + c;
                            if (i2 < n && j2 < n) ent[(size_t)(i2 * n + j2)] += 1;
                        } else if (i < n && j < n) {
                            ent[(size_t)(i * n + j)] += 1;
                        }
                    }
            }
        for (int v : ent) CHECK(v == 1);
    }
    return 0;
}

static int check_plans() {
    for (int64_t n : {INT64_C(1), INT64_C(2), INT64_C(63), INT64_C(64), INT64_C(65), INT64_C(255), INT64_C(256), INT64_C(257),
                      INT64_C(1023), INT64_C(1025), INT64_C(64800), INT64_C(1) << 17})
        for (int64_t d : {INT64_C(1), INT64_C(16), INT64_C(1280)})
            for (int64_t max_grid : {INT64_C(0), INT64_C(1), INT64_C(3), INT64_C(100000)}) {
                const ClusterPlan p = cluster_plan(n, d, max_grid);
                CHECK(p.valid && p.block == CLUSTER_BLOCK && p.serial_block == CLUSTER_SERIAL_BLOCK);
                CHECK(p.cap >= 1 && p.cap <= CLUSTER_MAX_GRID && (max_grid == 0 || p.cap <= max_grid));
                for (unsigned g : {p.norm_grid, p.fin_grid, p.scan_grid}) CHECK(g >= 1 && (int64_t)g <= p.cap);
                CHECK(p.matrix_bytes == (size_t)n * (size_t)n * 8 && p.matrix_bytes / 8 / (size_t)n == (size_t)n);
                // the workspace: regions in order, aligned, none overlapping, all inside
                const size_t off[] = {p.off_active, p.off_stale, p.off_mrow, p.off_nn, p.off_nnd, p.off_list, p.off_pi,
                                      p.off_pj, p.off_counters, p.ws_bytes};
                const size_t len[] = {(size_t)n, (size_t)n, (size_t)n, (size_t)n * 4, (size_t)n * 8, (size_t)n * 4,
                                      (size_t)(n / 2 + 1) * 4, (size_t)(n / 2 + 1) * 4, 64};
                for (int i = 0; i < 9; ++i) CHECK(off[i] % 8 == 0 && off[i] + len[i] <= off[i + 1]);
                // nothing of it depends on the grid
                const ClusterPlan q = cluster_plan(n, d, 0);
                CHECK(q.ws_bytes == p.ws_bytes && q.chunks == p.chunks && q.serial_rows == p.serial_rows && q.fin_items == p.fin_items);
                if (check_cover(p, n)) return 1;
            }
    // the design shape: a 1-degree grid
    {
        const ClusterPlan p = cluster_plan(64800, 256, 0);
        CHECK(p.matrix_bytes == (size_t)33592320000ULL && p.chunks == 64 && p.serial_rows == 64 && p.tiles == 1013);
        CHECK(p.scan_grid == CLUSTER_MAX_GRID && p.grid_of(5) == 5 && p.grid_of(0) == 1);
    }
    // refused
    CHECK(!cluster_plan(0, 16, 0).valid && !cluster_plan(-1, 16, 0).valid && !cluster_plan(CLUSTER_MAX_ROWS + 1, 16, 0).valid);
    CHECK(!cluster_plan(std::numeric_limits<int64_t>::max(), 16, 0).valid);
    CHECK(!cluster_plan(100, 0, 0).valid && !cluster_plan(100, CLUSTER_MAX_D + 1, 0).valid && !cluster_plan(100, 16, -1).valid);
    CHECK(cluster_plan(CLUSTER_MAX_ROWS, CLUSTER_MAX_D, 0).valid);
    return 0;
}

static bool labels_are(const std::vector<int32_t>& got, std::initializer_list<int32_t> want) {
    return got == std::vector<int32_t>(want);
}

static int check_cuts() {
    // five rows; emission order is not height order: (3, 4) at 1 is emitted after (0, 1) at 2
    const int32_t merges[] = {0, 1, 3, 4, 0, 2, 0, 3};
    const double heights[] = {2.0, 1.0, 3.0, 7.0};
    std::vector<int32_t> lab(5);
    std::vector<double> Z(16);
    CHECK(cluster_cut(5, merges, heights, 5, lab.data(), Z.data()) && labels_are(lab, {0, 1, 2, 3, 4}));
    // scipy's matrix: the sorted merges, ids of new clusters 5, 6, 7, 8
    const double wantZ[] = {3, 4, 1, 2, 0, 1, 2, 2, 2, 6, 3, 3, 5, 7, 7, 5};
    for (int i = 0; i < 16; ++i) CHECK(Z[(size_t)i] == wantZ[i]);
    CHECK(cluster_cut(5, merges, heights, 4, lab.data(), nullptr) && labels_are(lab, {0, 1, 2, 3, 3}));
    CHECK(cluster_cut(5, merges, heights, 3, lab.data(), nullptr) && labels_are(lab, {0, 0, 1, 2, 2}));
    CHECK(cluster_cut(5, merges, heights, 2, lab.data(), nullptr) && labels_are(lab, {0, 0, 0, 1, 1}));
    CHECK(cluster_cut(5, merges, heights, 1, lab.data(), nullptr) && labels_are(lab, {0, 0, 0, 0, 0}));
    CHECK(cluster_cut(5, merges, heights, 2, nullptr, Z.data()));            // either output alone
    // equal heights: the sort is stable, a parent emitted after its children stays behind them
    const int32_t m2[] = {0, 1, 2, 3, 0, 2, 4, 5, 0, 4};
    const double h2[] = {1.0, 1.0, 1.0, 1.0, 1.0};
    lab.assign(6, -1);
    Z.assign(20, 0.0);
    CHECK(cluster_cut(6, m2, h2, 3, lab.data(), Z.data()) && labels_are(lab, {0, 0, 0, 0, 1, 2}));
    CHECK(Z[8] == 6 && Z[9] == 7 && Z[11] == 4 && Z[16] == 8 && Z[17] == 9 && Z[19] == 6);
    CHECK(cluster_cut(6, m2, h2, 2, lab.data(), nullptr) && labels_are(lab, {0, 0, 0, 0, 1, 1}));
    // first occurrence: the cluster of row 0 is 0 whatever its rows' indices
    lab.assign(4, -1);
    const int32_t m4[] = {1, 3, 0, 2, 0, 1};
    const double h4[] = {1.0, 2.0, 3.0};
    CHECK(cluster_cut(4, m4, h4, 2, lab.data(), nullptr) && labels_are(lab, {0, 1, 0, 1}));
    CHECK(cluster_cut(4, m4, h4, 3, lab.data(), nullptr) && labels_are(lab, {0, 1, 2, 1}));
    // n = 2 and n = 1
    const int32_t m5[] = {0, 1};
    const double h5[] = {0.5};
    lab.assign(2, -1);
    CHECK(cluster_cut(2, m5, h5, 1, lab.data(), nullptr) && labels_are(lab, {0, 0}));
    CHECK(cluster_cut(2, m5, h5, 2, lab.data(), nullptr) && labels_are(lab, {0, 1}));
    lab.assign(1, -1);
    CHECK(cluster_cut(1, nullptr, nullptr, 1, lab.data(), nullptr) && labels_are(lab, {0}));
    // refused: k outside 1..n, rows outside 0..n-1, a merge inside one cluster, null records
    CHECK(!cluster_cut(5, merges, heights, 0, lab.data(), nullptr) && !cluster_cut(5, merges, heights, 6, lab.data(), nullptr));
    CHECK(!cluster_cut(0, merges, heights, 1, lab.data(), nullptr) && !cluster_cut(5, nullptr, heights, 2, lab.data(), nullptr));
    const int32_t bad1[] = {0, 5, 1, 2, 3, 4, 0, 1};
    const int32_t bad2[] = {0, 1, 1, 0, 2, 3, 0, 4};
    const int32_t bad3[] = {0, -1, 1, 2, 3, 4, 0, 1};
    lab.assign(5, -1);
    CHECK(!cluster_cut(5, bad1, heights, 2, lab.data(), nullptr) && !cluster_cut(5, bad2, heights, 2, lab.data(), nullptr));
    CHECK(!cluster_cut(5, bad3, heights, 2, lab.data(), nullptr));
    return 0;
}

int main() {
    if (check_plans() || check_cuts()) return 1;
    std::printf("cluster_plan ok block=%d tile=%d chunk=%d max_rows=%lld\n", CLUSTER_BLOCK, CLUSTER_TILE, CLUSTER_CHUNK,
                (long long)CLUSTER_MAX_ROWS);
    return 0;
}
