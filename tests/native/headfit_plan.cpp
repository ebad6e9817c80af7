// The launch plan of the class-head fit (range_amd/csrc/host_plan.h: headfit_plan) on the CPU, built with g++ under
// AddressSanitizer / UndefinedBehaviorSanitizer by tests/test_headfit_cpu.py.  For the GPU tests' shapes, with and
// without forced panels and grid caps: every (row, class) is covered exactly once by the gradient launches' items
// (row tile, chunk; every wave its tiles), every (class, feature) exactly once by the update launches' items
// (class tile, feature group; every wave its two feature tiles); every index the kernels form stays inside the
// workspace's parts; the workspace is at most 256 MiB; nothing overflows at C = 32768 with 8192 rows; the refusals.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../range_amd/csrc/host_plan.h"

using namespace range_host;

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); std::exit(1); } \
    } while (0)

static void check_sizes(const HeadfitPlan& p) {
    CHECK(p.valid && p.panel_tiles >= 1 && p.panel_cols == 32 * p.panel_tiles);
    CHECK((int64_t)p.n_panels * p.panel_tiles >= p.n_tiles && (int64_t)(p.n_panels - 1) * p.panel_tiles < p.n_tiles);
    CHECK(p.n_tiles * 32 >= p.C && (p.n_tiles - 1) * 32 < p.C);
    CHECK(p.row_tiles * p.tile_rows >= p.rows && (p.row_tiles - 1) * p.tile_rows < p.rows);
    CHECK(p.x_floats == (size_t)p.rows * p.F && p.g_floats == (size_t)p.rows * p.panel_cols);
    CHECK(p.part_floats == 2 * (size_t)p.panel_tiles * p.rows && p.rowsum_floats == 2 * (size_t)p.rows);
    CHECK(p.ws_bytes == 4 * (p.x_floats + p.g_floats + p.part_floats + p.rowsum_floats));
    CHECK(p.ws_bytes <= HEADFIT_MAX_WS);
    CHECK(p.lds_bytes == ((size_t)p.tile_rows * p.ld + p.tile_rows) * 4 && p.lds_bytes <= 160 * 1024);
    CHECK(p.ld % 2 == 1 && p.ld > p.k_groups * 8 && p.k_groups * 8 >= p.F);
    CHECK(p.f_groups * HEADFIT_FGROUP >= p.F && (p.f_groups - 1) * HEADFIT_FGROUP < p.F);
    CHECK(p.packed_floats == (size_t)p.n_tiles * 32 * p.k_groups * 8);
    // the largest indices the kernels form fit their 32-bit / 64-bit types with room
    CHECK((int64_t)p.rows * p.panel_cols < (INT64_C(1) << 31) && (int64_t)p.rows * p.F < (INT64_C(1) << 31));
    CHECK(p.packed_floats / 4 < (size_t)1 << 32);
    for (int pn = 0; pn < p.n_panels; ++pn) {
        CHECK(p.panel_n_tiles(pn) >= 1 && p.panel_n_tiles(pn) <= p.panel_tiles);
        CHECK(p.grad_grid(pn) >= 1 && (int64_t)p.grad_grid(pn) <= std::min(p.grad_items(pn), CSP_MAX_GRID));
        CHECK(p.update_grid(pn) >= 1 && (int64_t)p.update_grid(pn) <= std::min(p.update_items(pn), CSP_MAX_GRID));
        if (p.max_grid) CHECK((int64_t)p.grad_grid(pn) <= p.max_grid && (int64_t)p.update_grid(pn) <= p.max_grid);
    }
    CHECK(p.row_grid >= 1 && p.gather_grid >= 1 && p.unpack_grid >= 1);
}

static void check_cover(int C, int F, int64_t rows, int64_t cap, int panel_cols) {
    const HeadfitPlan p = headfit_plan(C, F, rows, cap, panel_cols);
    check_sizes(p);
    if (panel_cols) CHECK(p.panel_cols == std::min((panel_cols + 31) / 32, p.n_tiles) * 32);
    std::vector<unsigned char> hit((size_t)rows * C, 0), upd((size_t)C * F, 0);
    int tiles = 0;
    for (int pn = 0; pn < p.n_panels; ++pn) {
        const int tile0 = p.panel_first_tile(pn), n = p.panel_n_tiles(pn);
        CHECK(tile0 == tiles);
        tiles += n;
        // the gradient launch, workgroup by workgroup, grid-stride
        const unsigned grid = p.grad_grid(pn);
        for (unsigned blk = 0; blk < grid; ++blk)
            for (int64_t it = blk; it < p.grad_items(pn); it += grid) {
                int64_t rt;
                int ch;
                p.grad_item(pn, it, rt, ch);
                CHECK(rt >= 0 && rt < p.row_tiles && ch >= 0 && ch < p.grad_chunks(pn));
                for (int w = 0; w < 4; ++w)
                    for (int j = 0; j < p.wave_n_tiles(pn, ch, w); ++j) {
                        const int lt = p.wave_first_tile(ch, w) + 4 * j;
                        CHECK(lt < n);
                        // G and the two row sums of this tile: inside their parts of the workspace
                        CHECK((size_t)(rows - 1) * p.panel_cols + lt * 32 + 31 < p.g_floats);
                        CHECK(((size_t)p.panel_tiles + lt) * rows + rows - 1 < p.part_floats);
                        for (int c = (tile0 + lt) * 32; c < (tile0 + lt) * 32 + 32 && c < C; ++c)
                            for (int64_t r = rt * p.tile_rows; r < (rt + 1) * p.tile_rows && r < rows; ++r) {
                                CHECK(hit[(size_t)r * C + c] == 0);
                                hit[(size_t)r * C + c] = 1;
                            }
                    }
            }
        // the update launch: item = class tile x feature group, wave w features (4 fg + w) 64 .. + 63
        const unsigned ug = p.update_grid(pn);
        for (unsigned blk = 0; blk < ug; ++blk)
            for (int64_t it = blk; it < p.update_items(pn); it += ug) {
                const int lt = (int)(it / p.f_groups), fg = (int)(it - (int64_t)lt * p.f_groups);
                CHECK(lt < n);
                for (int w = 0; w < 4; ++w) {
                    const int fb = (fg * 4 + w) * 64;
                    for (int f = fb; f < fb + 64 && f < F; ++f) {
                        CHECK(f / 8 < p.k_groups);
                        for (int c = (tile0 + lt) * 32; c < (tile0 + lt) * 32 + 32 && c < C; ++c) {
                            CHECK(upd[(size_t)c * F + f] == 0);
                            upd[(size_t)c * F + f] = 1;
                        }
                    }
                }
            }
    }
    CHECK(tiles == p.n_tiles);
    for (unsigned char h : hit) CHECK(h == 1);
    for (unsigned char h : upd) CHECK(h == 1);
}

int main() {
    // the GPU tests' shapes (B + Bg, C, F), with the plan's panel and forced ones, with and without a grid cap
    const int shapes[][3] = {{1, 1, 1}, {2, 2, 3}, {64, 33, 7}, {64, 32, 8}, {64, 65, 9}, {128, 70, 40}, {128, 129, 257},
                             {96, 257, 520}, {5, 8142, 16}, {96, 70, 40}, {66, 33, 24}};
    for (const auto& s : shapes)
        for (int64_t cap : {INT64_C(0), INT64_C(1), INT64_C(2)})
            for (int panel : {0, 1, 32, 33, 64, 100}) check_cover(s[1], s[2], s[0], cap, panel);
    check_cover(300, 1024, 200, 0, 96);
    // the design shape and the envelope's corner: sizes only
    {
        const HeadfitPlan d = headfit_plan(8142, 256, 2048);
        check_sizes(d);
        CHECK(d.n_panels == 1 && d.panel_cols == 8160 && d.tile_rows == 64 && d.cols_per_pass == 256 && d.f_groups == 1);
        CHECK(d.grad_items(0) == 32 * 32 && d.update_items(0) == 255);
        std::printf("headfit_plan(8142, 256, 2048): ws_bytes = %zu\n", d.ws_bytes);
        const HeadfitPlan big = headfit_plan(32768, 1024, 8192);
        check_sizes(big);
        CHECK(big.n_panels > 1 && big.tile_rows == 32 && big.cols_per_pass == 512 && big.f_groups == 4);
        std::printf("headfit_plan(32768, 1024, 8192): panel_cols = %d, n_panels = %d, ws_bytes = %zu\n", big.panel_cols, big.n_panels,
                    big.ws_bytes);
        check_sizes(headfit_plan(32768, 1, 8192));
        check_sizes(headfit_plan(1, 1024, 8192));
        check_sizes(headfit_plan(32768, 1024, 8192, 3, 32));
    }
    // refusals
    CHECK(!headfit_plan(0, 8, 8).valid && !headfit_plan(32769, 8, 8).valid);
    CHECK(!headfit_plan(8, 0, 8).valid && !headfit_plan(8, 1025, 8).valid);
    CHECK(!headfit_plan(8, 8, 0).valid && !headfit_plan(8, 8, 8193).valid);
    CHECK(!headfit_plan(8, 8, 8, -1).valid && !headfit_plan(8, 8, 8, 0, -1).valid);
    CHECK(*headfit_plan(8, 8, 8193).why != 0);
    std::printf("headfit_plan ok\n");
    return 0;
}
