// The launch plan and the weight packing of the CSP location encoders (range_amd/csrc/host_plan.h: csp_plan,
// csp_packed_index, csp_pack_layer) on the CPU, built with g++ under AddressSanitizer /
// UndefinedBehaviorSanitizer by tests/test_csp_cpu.py: tile height, grid, LDS bytes, padded widths and the
// packed size over the envelope; every index the kernel forms (csp_kernel.h) inside the LDS image and the
// packed parameters; every weight packed exactly once and found where the kernel's lane reads it; the tiles
// of a launch covered exactly once, also with a capped grid and beyond 2^31 locations; the invalid cases.
// The width lists of tests/csp_sweep_cases.py (SWEEP; `csp_plan --sweep` prints this file's copy, which
// tests/test_csp_sweep_cpu.py compares with that table): the tile height, and the packing read back through
// csp_packed_index - every (n, k) at an index of its own inside the layer's weights, every other float zero.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../range_amd/csrc/host_plan.h"

using namespace range_host;

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); std::exit(1); } \
    } while (0)

static void check_network(int kind, int F, const std::vector<int>& widths, bool skip, bool layn) {
    const int n = (int)widths.size();
    const CspPlan p = csp_plan(kind, F, n, widths.data(), skip, layn, 1);
    CHECK(p.valid && p.n_layers == n && p.in0 == posenc_per_freq(kind) * F && p.out_width == widths.back());
    int widest = p.in0;
    for (int w : widths) widest = std::max(widest, w);
    CHECK(p.m_tiles == (widest <= 512 ? 2 : 1) && p.tile_rows == 32 * p.m_tiles && p.block == CSP_BLOCK);
    CHECK(p.ld % 2 == 1 && p.ld > widest && p.lds_bytes == (size_t)p.tile_rows * p.ld * 4);
    CHECK(p.lds_bytes <= 160 * 1024);                       // the CU's LDS
    size_t end = 0;
    int in = p.in0;
    for (int i = 0; i < n; ++i) {
        const CspLayerPlan& l = p.layer[i];
        CHECK(l.in == in && l.out == widths[i]);
        CHECK(l.k_pad() >= l.in && l.k_pad() - l.in < CSP_KGROUP && l.n_pad() >= l.out && l.n_pad() - l.out < CSP_NTILE);
        CHECK(l.k_pad() < p.ld && l.n_pad() < p.ld);         // the A operand's and the epilogue's columns are in the row
        CHECK((l.n_tiles + 3) / 4 * p.m_tiles <= CSP_ACC_TILES);   // a wave's share fits its accumulators
        const bool hidden = i + 1 < n;
        CHECK(l.skip == (hidden && skip && l.in == l.out) && l.layn == (hidden && layn));
        CHECK(l.w_off == end && l.w_off % 4 == 0);           // 16-byte fragments
        end += (size_t)l.k_pad() * l.n_pad();
        CHECK(l.b_off == end);
        end += l.n_pad();
        if (l.layn) { CHECK(l.g_off == end && l.be_off == end + l.n_pad()); end += 2 * (size_t)l.n_pad(); }
        in = l.out;
    }
    CHECK(p.packed_floats == end && end < (size_t)1 << 32);
    // pack: weight (n, k) = 1 + n * in + k, found again at the place lane `lane` of step `s` reads
    std::vector<float> packed(p.packed_floats, 0.0f);
    for (int i = 0; i < n; ++i) {
        const CspLayerPlan& l = p.layer[i];
        std::vector<float> w((size_t)l.out * l.in), b(l.out), g(l.out), be(l.out);
        for (size_t j = 0; j < w.size(); ++j) w[j] = (float)(1 + j);
        for (int j = 0; j < l.out; ++j) { b[j] = -1.0f - j; g[j] = 0.5f + j; be[j] = -0.25f - j; }
        csp_pack_layer(p, i, w.data(), b.data(), g.data(), be.data(), packed.data());
        size_t nonzero = 0;
        for (int nt = 0; nt < l.n_tiles; ++nt)
            for (int kg = 0; kg < l.k_groups; ++kg)
                for (int lane = 0; lane < 64; ++lane)
                    for (int s = 0; s < 4; ++s) {
                        const size_t at = l.w_off + (((size_t)nt * l.k_groups + kg) * 64 + lane) * 4 + s;
                        CHECK(at < l.b_off);
                        const int col = nt * 32 + (lane & 31), k = kg * 8 + 2 * s + (lane >> 5);
                        const float want = col < l.out && k < l.in ? (float)(1 + (size_t)col * l.in + k) : 0.0f;
                        CHECK(packed[at] == want);
                        nonzero += want != 0.0f;
                    }
        CHECK(nonzero == w.size());
        for (int j = 0; j < l.n_pad(); ++j) {
            CHECK(packed[l.b_off + j] == (j < l.out ? b[j] : 0.0f));
            if (l.layn) CHECK(packed[l.g_off + j] == (j < l.out ? g[j] : 0.0f) && packed[l.be_off + j] == (j < l.out ? be[j] : 0.0f));
        }
    }
}

static void check_tiles(const CspPlan& p, int64_t B) {
    CHECK(p.valid && p.grid >= 1 && (int64_t)p.grid <= CSP_MAX_GRID && (int64_t)p.grid <= p.n_tiles);
    CHECK(p.n_tiles * p.tile_rows >= B && (p.n_tiles - 1) * p.tile_rows < B);
    int64_t sum = 0;
    for (int64_t blk = 0; blk < (int64_t)p.grid; ++blk) sum += p.tiles_of(blk);
    CHECK(sum == p.n_tiles && p.tiles_of(p.n_tiles) == 0);
}

struct SweepCase { const char* name; int kind, F; std::vector<int> widths; bool skip, layn; int tile_rows; };

static const std::vector<SweepCase>& sweep_cases() {
    static const std::vector<SweepCase> cases = {
        {"t32_sigmoid", PE_GRID, 3, {520, 520, 33}, true, true, 32},
        {"t32_relu_1024", PE_THEORY, 64, {1024, 1}, false, false, 32},
        {"t32_leaky_mixed", PE_GRID, 1, {40, 600, 600, 24}, true, true, 32},
        {"t32_tanh_1024sq", PE_THEORY, 5, {1024, 1024, 7}, true, true, 32},
        {"t32_gelu_513", PE_GRID, 16, {513, 31}, true, true, 32},
        {"t64_deep9", PE_GRID, 2, {8, 8, 8, 8, 8, 8, 8, 8, 8}, true, true, 64},
        {"t64_deep9_plain", PE_THEORY, 4, {24, 24, 24, 24, 24, 24, 24, 24, 5}, true, false, 64},
        {"t64_mixed", PE_THEORY, 7, {512, 9, 33, 33, 512, 9}, true, true, 64},
        {"t64_F64", PE_GRID, 64, {256, 256, 100}, true, false, 64},
        {"t64_w1", PE_GRID, 1, {1}, false, false, 64},
        {"saturated", PE_GRID, 8, {64, 16}, false, false, 64},
    };
    return cases;
}

// W[n][k] = 1 + n * in + k (exact in float32 up to 1024 x 1024) packed and read back: every (n, k) at an index of
// its own inside [w_off, b_off), every other float of the layer's weights zero; the other layers' floats untouched
static void check_sweep_packing(const SweepCase& c) {
    const int n_layers = (int)c.widths.size();
    const CspPlan p = csp_plan(c.kind, c.F, n_layers, c.widths.data(), c.skip, c.layn, 1);
    CHECK(p.valid && p.tile_rows == c.tile_rows && p.m_tiles * 32 == c.tile_rows);
    for (int i = 0; i < n_layers; ++i) {
        const CspLayerPlan& l = p.layer[i];
        std::vector<float> packed(p.packed_floats, 0.0f);
        std::vector<float> w((size_t)l.out * l.in), b(l.out, 0.0f), g(l.out, 0.0f), be(l.out, 0.0f);
        for (size_t j = 0; j < w.size(); ++j) w[j] = (float)(1 + j);
        csp_pack_layer(p, i, w.data(), b.data(), g.data(), be.data(), packed.data());
        std::vector<char> seen(p.packed_floats, 0);
        for (int n = 0; n < l.out; ++n)
            for (int k = 0; k < l.in; ++k) {
                const size_t at = l.w_off + csp_packed_index(l, n, k);
                CHECK(at >= l.w_off && at < l.b_off && !seen[at]);
                seen[at] = 1;
                CHECK(packed[at] == (float)(1 + (size_t)n * l.in + k));
            }
        for (size_t at = 0; at < p.packed_floats; ++at) CHECK(seen[at] || packed[at] == 0.0f);
    }
}

static void print_sweep() {
    for (const SweepCase& c : sweep_cases()) {
        const int n_layers = (int)c.widths.size();
        const CspPlan p = csp_plan(c.kind, c.F, n_layers, c.widths.data(), c.skip, c.layn, 1);
        std::printf("%s kind=%s F=%d skip=%d layn=%d T=%d layers=%d widths=", c.name, c.kind == PE_GRID ? "gridcell" : "theory",
                    c.F, (int)c.skip, (int)c.layn, p.tile_rows, n_layers);
        for (int i = 0; i < n_layers; ++i) std::printf("%s%d", i ? "," : "", c.widths[i]);
        std::printf(" ntw=");        // column tiles of wave 0 (the largest share) per layer
        for (int i = 0; i < n_layers; ++i) std::printf("%s%d", i ? "," : "", (p.layer[i].n_tiles + 3) / 4);
        std::printf(" idle_waves=");
        for (int i = 0; i < n_layers; ++i) std::printf("%s%d", i ? "," : "", std::max(0, 4 - p.layer[i].n_tiles));
        std::printf("\n");
    }
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "--sweep")) { print_sweep(); return 0; }
    for (const SweepCase& c : sweep_cases()) {
        check_network(c.kind, c.F, c.widths, c.skip, c.layn);
        check_sweep_packing(c);
    }
    for (int kind : {PE_GRID, PE_THEORY})
        for (int F : {1, 5, 16, 32, 64})
            for (bool skip : {false, true})
                for (bool layn : {false, true}) {
                    check_network(kind, F, {256}, skip, layn);
                    check_network(kind, F, {512, 256}, skip, layn);
                    check_network(kind, F, {posenc_per_freq(kind) * F, 7}, skip, layn);
                    check_network(kind, F, {40, 40, 24}, skip, layn);
                    check_network(kind, F, {1, 1}, skip, layn);
                }
    check_network(PE_GRID, 32, {1024, 1024, 1024}, true, true);
    check_network(PE_THEORY, 64, {513, 33, 1024}, true, true);
    check_network(PE_GRID, 64, {96, 96, 96, 96, 96, 96, 96, 96, 256}, true, true);       // 8 hidden layers
    const int design[2] = {512, 256};
    {
        const CspPlan p = csp_plan(PE_GRID, 32, 2, design, true, true, 1);
        CHECK(p.tile_rows == 64 && p.ld == 513 && p.lds_bytes == 64 * 513 * 4 && p.packed_floats == 128 * 512 + 512 * 3 + 512 * 256 + 256);
    }
    for (int64_t B : {INT64_C(1), INT64_C(63), INT64_C(64), INT64_C(65), INT64_C(131), INT64_C(1000000), (INT64_C(1) << 31) + 5,
                      INT64_C(1) << 48}) {
        check_tiles(csp_plan(PE_GRID, 32, 2, design, true, true, B), B);
        for (int64_t cap : {INT64_C(1), INT64_C(2), INT64_C(3), INT64_C(5000)}) {
            const CspPlan p = csp_plan(PE_GRID, 32, 2, design, true, true, B, cap);
            check_tiles(p, B);
            CHECK((int64_t)p.grid <= cap);
        }
    }
    {
        const CspPlan p = csp_plan(PE_GRID, 32, 2, design, true, true, (INT64_C(1) << 31) + 5);
        CHECK((int64_t)p.grid == CSP_MAX_GRID && p.tiles_of(0) > 1);
    }
    // outside the envelope
    const int wide[1] = {1025}, zero[1] = {0}, ten[10] = {8, 8, 8, 8, 8, 8, 8, 8, 8, 8};
    CHECK(!csp_plan(PE_SPHEREC, 32, 2, design, true, true, 1).valid && !csp_plan(-1, 32, 2, design, true, true, 1).valid);
    CHECK(!csp_plan(PE_GRID, 0, 2, design, true, true, 1).valid && !csp_plan(PE_GRID, 65, 2, design, true, true, 1).valid);
    CHECK(!csp_plan(PE_GRID, 32, 1, wide, true, true, 1).valid && !csp_plan(PE_GRID, 32, 1, zero, true, true, 1).valid);
    CHECK(!csp_plan(PE_GRID, 32, 10, ten, true, true, 1).valid && !csp_plan(PE_GRID, 32, 0, design, true, true, 1).valid);
    CHECK(csp_plan(PE_GRID, 32, 9, ten, true, true, 1).valid && !csp_plan(PE_GRID, 32, 2, nullptr, true, true, 1).valid);
    CHECK(!csp_plan(PE_GRID, 32, 2, design, true, true, 0).valid && !csp_plan(PE_GRID, 32, 2, design, true, true, -4).valid);
    CHECK(!csp_plan(PE_GRID, 32, 2, design, true, true, std::numeric_limits<int64_t>::max()).valid);
    CHECK(!csp_plan(PE_GRID, 32, 2, design, true, true, 10, -1).valid);
    CHECK(*csp_plan(PE_GRID, 65, 2, design, true, true, 1).why != 0);
    std::printf("csp_plan ok\n");
    return 0;
}
