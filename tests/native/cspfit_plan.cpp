// The launch plan of the CSP encoder fit (range_amd/csrc/host_plan.h: cspfit_plan) on the CPU, built with g++ under
// AddressSanitizer / UndefinedBehaviorSanitizer by tests/test_cspfit_cpu.py.  For the GPU tests' shapes, with and
// without forced panels and grid caps: the row launches' groups cover every row once; the items of dX = dZ W / dE = G W_c
// cover every (row, column) once; the column sums' threads every (kind, column) once; the layers' dW launches every
// (output, input) once; the forward products are csp_head_plan's (tests/native/csp_head_plan.cpp covers them); the
// parts of the workspace and of the parameter store are disjoint, in order and inside their totals; the workspace is at
// most 512 MiB and a shape beyond it is refused.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../range_amd/csrc/host_plan.h"

using namespace range_host;

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); std::exit(1); } \
    } while (0)

static void check_offsets(const CspfitPlan& p) {
    // the workspace: features, then per layer Z and the output, the four gradient images, the head's three parts
    size_t at = 0;
    CHECK(p.x_off[0] == at);
    at += (size_t)p.rows * p.net.in0;
    for (int l = 0; l < p.n_layers; ++l) {
        CHECK(p.z_off[l] == at); at += (size_t)p.rows * p.out(l);
        CHECK(p.x_off[l + 1] == at); at += (size_t)p.rows * p.out(l);
        CHECK(p.widest >= p.in(l) && p.widest >= p.out(l));
    }
    for (int i = 0; i < 2; ++i) { CHECK(p.dy_off[i] == at); at += (size_t)p.rows * p.widest; }
    CHECK(p.dz_off == at); at += (size_t)p.rows * p.widest;
    CHECK(p.dyx_off == at); at += (size_t)p.rows * p.widest;
    CHECK(p.g_ws_off == at); at += p.head.g_floats;
    CHECK(p.part_off == at); at += p.head.part_floats;
    CHECK(p.rowsum_off == at); at += p.head.rowsum_floats;
    CHECK(p.ws_floats == at && p.ws_bytes == 4 * at && p.ws_bytes <= CSPFIT_MAX_WS);
    // the stores
    size_t s = 0, u = 0;
    for (int l = 0; l < p.n_layers; ++l) {
        const CspLayerPlan& L = p.net.layer[l];
        CHECK(p.w_off[l] == s && s % 4 == 0); s += p.fwd(l).packed_floats;
        CHECK(p.fwd(l).packed_floats == p.upd(l).packed_floats && p.fwd(l).k_groups == p.upd(l).k_groups);
        CHECK(p.b_off[l] == s); s += L.n_pad();
        if (L.layn) { CHECK(p.g_off[l] == s && p.be_off[l] == s + L.n_pad()); s += 2 * (size_t)L.n_pad(); }
        CHECK(p.uw_off[l] == u); u += (size_t)L.out * L.in;
        CHECK(p.ub_off[l] == u); u += L.out;
        if (L.layn) { CHECK(p.ug_off[l] == u && p.ube_off[l] == u + L.out); u += 2 * (size_t)L.out; }
        CHECK(p.upd(l).valid && p.upd(l).n_panels == 1 && p.fwd(l).valid);
        CHECK(p.fwd(l).lds_bytes <= p.lds_bytes && p.lds_bytes <= 160 * 1024);
    }
    CHECK(p.c_off == s && s % 4 == 0); s += p.head.packed_floats;
    CHECK(p.uc_off == u); u += (size_t)p.C * p.net.out_width;
    CHECK(p.store_floats == s && p.n_params == u);
    CHECK(p.lpr == 4 || p.lpr == 8);
    CHECK(p.lpr * p.rows_per_wg == CSP_BLOCK && p.rows_per_wg == p.net.tile_rows);
    CHECK(p.feat_grid >= 1 && p.row_grid >= 1);
    if (p.max_grid) CHECK((int64_t)p.feat_grid <= p.max_grid && (int64_t)p.row_grid <= p.max_grid);
}

static void check_cover(int kind, int F, int n_layers, const int* widths, bool skip, bool layn, int C, int64_t rows, int64_t cap,
                        int panel_cols) {
    const CspfitPlan p = cspfit_plan(kind, F, n_layers, widths, skip, layn, C, rows, cap, panel_cols);
    CHECK(p.valid);
    check_offsets(p);
    // the row launches: group g = rows g * rows_per_wg .., thread t its row t / lpr
    {
        std::vector<unsigned char> hit(rows, 0);
        const int64_t groups = (rows + p.rows_per_wg - 1) / p.rows_per_wg;
        for (unsigned blk = 0; blk < p.row_grid; ++blk)
            for (int64_t g = blk; g < groups; g += p.row_grid)
                for (int t = 0; t < CSP_BLOCK; t += p.lpr) {
                    const int64_t r = g * p.rows_per_wg + t / p.lpr;
                    if (r < rows) { CHECK(hit[r] == 0); hit[r] = 1; }
                }
        for (unsigned char h : hit) CHECK(h == 1);
    }
    // dX / dE on `cols` columns, and the layers' column sums and dW
    std::vector<int> col_counts = {p.net.out_width};
    for (int l = 1; l < n_layers; ++l) col_counts.push_back(p.in(l));
    for (int cols : col_counts) {
        std::vector<unsigned char> hit((size_t)rows * cols, 0);
        const unsigned grid = p.back_grid(cols);
        CHECK(grid >= 1 && (int64_t)grid <= p.back_items(cols));
        if (cap) CHECK((int64_t)grid <= cap);
        for (unsigned blk = 0; blk < grid; ++blk)
            for (int64_t it = blk; it < p.back_items(cols); it += grid) {
                const int64_t rt = it / p.back_col_groups(cols);
                const int cg = (int)(it - rt * p.back_col_groups(cols));
                for (int w = 0; w < 4; ++w)
                    for (int c = (cg * 4 + w) * 32; c < (cg * 4 + w) * 32 + 32 && c < cols; ++c)
                        for (int64_t r = rt * 32; r < rt * 32 + 32 && r < rows; ++r) {
                            CHECK(hit[(size_t)r * cols + c] == 0);
                            hit[(size_t)r * cols + c] = 1;
                        }
            }
        for (unsigned char h : hit) CHECK(h == 1);
    }
    for (int l = 0; l < n_layers; ++l) {
        const int total = p.colsum_kinds(l) * p.out(l);
        std::vector<unsigned char> hit(total, 0);
        const unsigned grid = p.colsum_grid(l);
        CHECK(grid >= 1);
        for (unsigned blk = 0; blk < grid; ++blk)
            for (int t = 0; t < CSPFIT_COLSUM_BLOCK; ++t)
                for (int idx = blk * CSPFIT_COLSUM_BLOCK + t; idx < total; idx += grid * CSPFIT_COLSUM_BLOCK) {
                    CHECK(hit[idx] == 0);
                    hit[idx] = 1;
                }
        for (unsigned char h : hit) CHECK(h == 1);
        const HeadfitPlan u = p.upd(l);
        std::vector<unsigned char> upd((size_t)p.out(l) * p.in(l), 0);
        const unsigned ug = u.update_grid(0);
        for (unsigned blk = 0; blk < ug; ++blk)
            for (int64_t it = blk; it < u.update_items(0); it += ug) {
                const int lt = (int)(it / u.f_groups), fg = (int)(it - (int64_t)lt * u.f_groups);
                for (int w = 0; w < 4; ++w)
                    for (int f = (fg * 4 + w) * 64; f < (fg * 4 + w) * 64 + 64 && f < p.in(l); ++f)
                        for (int c = lt * 32; c < lt * 32 + 32 && c < p.out(l); ++c) {
                            CHECK(upd[(size_t)c * p.in(l) + f] == 0);
                            upd[(size_t)c * p.in(l) + f] = 1;
                        }
            }
        for (unsigned char h : upd) CHECK(h == 1);
    }
}

int main() {
    // the GPU tests' networks: (kind, F, widths...), rows, C
    struct Net { int kind, F, n; int w[4]; bool skip, layn; };
    const Net nets[] = {{PE_GRID, 4, 2, {16, 12}, true, true},   {PE_GRID, 4, 2, {20, 12}, true, false}, {PE_THEORY, 3, 3, {18, 18, 10}, true, true},
                        {PE_GRID, 5, 1, {14}, true, true},       {PE_GRID, 4, 4, {16, 16, 16, 12}, true, true}, {PE_GRID, 1, 2, {1, 1}, true, true},
                        {PE_GRID, 8, 2, {31, 33}, false, true},  {PE_GRID, 8, 2, {96, 33}, true, true},  {PE_THEORY, 1, 2, {513, 31}, true, true},
                        {PE_GRID, 24, 2, {96, 96}, true, true}};
    const int64_t row_counts[] = {1, 2, 31, 32, 33, 65, 96};
    const int classes[] = {1, 33, 70};
    for (const Net& n : nets)
        for (int64_t rows : row_counts)
            for (int C : classes)
                for (int64_t cap : {INT64_C(0), INT64_C(1)})
                    for (int panel : {0, 32}) check_cover(n.kind, n.F, n.n, n.w, n.skip, n.layn, C, rows, cap, panel);
    {
        // the design shape and the envelope: sizes only
        const int w1[] = {512, 256}, w3[] = {512, 512, 512, 256};
        const CspfitPlan d = cspfit_plan(PE_GRID, 32, 2, w1, true, true, 8142, 2048);
        CHECK(d.valid && d.head.n_panels == 1 && d.lpr == 4 && d.widest == 512);
        check_offsets(d);
        std::printf("cspfit_plan(design, 2048 rows): ws_bytes = %zu, n_params = %zu\n", d.ws_bytes, d.n_params);
        const CspfitPlan d3 = cspfit_plan(PE_GRID, 32, 4, w3, true, true, 8142, 2048);
        CHECK(d3.valid);
        check_offsets(d3);
        const int wide[] = {1024, 1024};
        const CspfitPlan big = cspfit_plan(PE_THEORY, 64, 2, wide, true, true, 32768, 4096);
        CHECK(big.valid && big.lpr == 8 && big.head.n_panels > 1);
        check_offsets(big);
        std::printf("cspfit_plan(1024 wide, C = 32768, 4096 rows): ws_bytes = %zu\n", big.ws_bytes);
        // 8192 rows of two 1024-wide layers, or of nine: the saved activations alone exceed the cap
        CHECK(!cspfit_plan(PE_THEORY, 64, 2, wide, true, true, 32768, 8192).valid);
        const int deep[] = {1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024};
        const CspfitPlan no = cspfit_plan(PE_THEORY, 64, 9, deep, true, true, 70, 8192);
        CHECK(!no.valid && *no.why != 0);
        CHECK(cspfit_plan(PE_THEORY, 64, 9, deep, true, true, 70, 512).valid);
    }
    // refusals
    const int w[] = {16, 12};
    CHECK(!cspfit_plan(PE_GRID, 4, 2, w, true, true, 70, 0).valid && !cspfit_plan(PE_GRID, 4, 2, w, true, true, 70, 8193).valid);
    CHECK(!cspfit_plan(PE_GRID, 65, 2, w, true, true, 70, 8).valid && !cspfit_plan(PE_GRID, 4, 2, w, true, true, 0, 8).valid);
    CHECK(!cspfit_plan(PE_GRID, 4, 2, w, true, true, 32769, 8).valid && !cspfit_plan(PE_SPHEREC, 4, 2, w, true, true, 70, 8).valid);
    CHECK(!cspfit_plan(PE_GRID, 4, 2, w, true, true, 70, 8, -1).valid && !cspfit_plan(PE_GRID, 4, 2, w, true, true, 70, 8, 0, -1).valid);
    const int bad[] = {1025, 12};
    CHECK(!cspfit_plan(PE_GRID, 4, 2, bad, true, true, 70, 8).valid && !cspfit_plan(PE_GRID, 4, 10, w, true, true, 70, 8).valid);
    std::printf("cspfit_plan ok\n");
    return 0;
}
