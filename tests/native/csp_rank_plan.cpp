// The launch plan of the CSP evaluation kernel (range_amd/csrc/host_plan.h: csp_rank_plan) on the CPU, built with
// g++ under AddressSanitizer / UndefinedBehaviorSanitizer by tests/test_csp_rank_cpu.py.  At the corners of the
// envelope: the tile and the chunks are the head's; the work items of a launch - walked grid-stride by the
// workgroups, every part its chunks, every wave its column tiles - cover B x C exactly once, with every col_parts
// and with a capped grid; the LDS image fits a CU (two workgroups at the design width); the workspace holds the
// parts; the refusals name a reason.
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

static void check_cover(int K, int C, int64_t B, int img, bool head, int64_t cap, int parts, bool count_cells) {
    const CspRankPlan p = csp_rank_plan(K, C, B, img, head, cap, parts);
    CHECK(p.valid && p.grid >= 1 && (int64_t)p.grid <= CSP_MAX_GRID && (int64_t)p.grid <= p.n_items);
    if (cap) CHECK((int64_t)p.grid <= cap);
    const CspHeadPlan h = csp_head_plan(K, C, C, B, CSP_HEAD_PROBS);
    if (head) {
        CHECK(p.m_tiles == h.m_tiles && p.tile_rows == h.tile_rows && p.ld == h.ld && p.k_groups == h.k_groups);
        CHECK(p.cols_per_pass == h.cols_per_pass && p.n_chunks == h.n_chunks && p.wave_tiles == h.wave_tiles);
    } else {
        CHECK(p.m_tiles == 2 && p.tile_rows == 64 && p.cols_per_pass == 256);
    }
    CHECK(p.col_tiles == h.col_tiles);
    CHECK(p.row_tiles * p.tile_rows >= B && (p.row_tiles - 1) * p.tile_rows < B);
    CHECK((int64_t)p.n_chunks * p.cols_per_pass >= C && (int64_t)(p.n_chunks - 1) * p.cols_per_pass < C);
    CHECK(p.col_parts >= 1 && p.col_parts <= p.n_chunks && p.n_items == p.row_tiles * p.col_parts);
    if (parts) CHECK(p.col_parts == parts);
    else CHECK(p.col_parts == p.n_chunks || (p.n_items >= CSP_RANK_TARGET_WG && (p.col_parts - 1) * p.row_tiles < CSP_RANK_TARGET_WG));
    CHECK(p.lds_bytes == (head ? (size_t)p.tile_rows * p.ld * 4 : 0) + (size_t)p.tile_rows * CSP_RANK_ROW_STATE);
    CHECK(p.lds_bytes <= 160 * 1024 && p.lds_bytes % 8 == 0 && ((size_t)p.tile_rows * p.ld * 4) % 16 == 0);
    if (p.col_parts > 1) CHECK(p.ws_bytes == (size_t)p.col_parts * (size_t)B * 20 && p.merge_grid >= 1);
    else CHECK(p.ws_bytes == 0 && p.merge_grid == 0);
    int64_t sum = 0;
    for (int64_t blk = 0; blk < (int64_t)p.grid; ++blk) sum += p.items_of(blk);
    CHECK(sum == p.n_items && p.items_of(p.n_items) == 0);
    // the parts of a row tile: consecutive, none empty, all chunks
    for (int64_t rt : {INT64_C(0), p.row_tiles - 1}) {
        int next = 0;
        for (int part = 0; part < p.col_parts; ++part) {
            int64_t r;
            int q, ch0, ch1;
            p.item(rt * p.col_parts + part, r, q, ch0, ch1);
            CHECK(r == rt && q == part && ch0 == next && ch1 > ch0);
            next = ch1;
        }
        CHECK(next == p.n_chunks);
    }
    if (!count_cells) return;
    std::vector<unsigned char> hit((size_t)B * (size_t)C, 0);
    for (int64_t blk = 0; blk < (int64_t)p.grid; ++blk)
        for (int64_t it = blk; it < p.n_items; it += p.grid) {
            int64_t rt;
            int part, ch0, ch1;
            p.item(it, rt, part, ch0, ch1);
            for (int ch = ch0; ch < ch1; ++ch)
                for (int w = 0; w < 4; ++w) {
                    const int n = p.wave_n_tiles(ch, w);
                    CHECK(n >= 0 && n <= p.wave_tiles);
                    for (int j = 0; j < n; ++j) {
                        const int tile = p.wave_first_tile(ch, w) + 4 * j;
                        CHECK(tile < p.col_tiles);
                        for (int c = tile * 32; c < tile * 32 + 32 && c < C; ++c)
                            for (int64_t r = rt * p.tile_rows; r < (rt + 1) * p.tile_rows && r < B; ++r) {
                                CHECK(hit[(size_t)r * C + c] == 0);
                                hit[(size_t)r * C + c] = 1;
                            }
                    }
                }
        }
    for (unsigned char hc : hit) CHECK(hc == 1);
}

int main() {
    for (int K : {24, 256, 600})
        for (int C : {1, 5, 31, 32, 33, 255, 256, 257, 513, 1025}) {
            const int chunks = csp_rank_plan(K, C, 1, CSP_IMG_F32, true).n_chunks;
            for (int64_t B : {INT64_C(1), INT64_C(31), INT64_C(33), INT64_C(64), INT64_C(65), INT64_C(129)})
                for (int64_t cap : {INT64_C(0), INT64_C(1), INT64_C(3)})
                    for (int parts : {0, 1, 2, chunks}) {
                        if (parts > chunks) continue;
                        check_cover(K, C, B, CSP_IMG_F32, true, cap, parts, true);
                        check_cover(K, C, B, CSP_IMG_F64, false, cap, parts, B == 65);
                    }
        }
    {
        // iNat-2018 val behind the design network: two workgroups a CU
        const CspRankPlan d = csp_rank_plan(256, 8142, 24426, CSP_IMG_F32, true);
        CHECK(d.valid && d.tile_rows == 64 && d.ld == 257 && d.cols_per_pass == 256 && d.n_chunks == 32 && d.row_tiles == 382);
        CHECK(d.col_parts == 2 && d.n_items == 764 && d.grid == 764 && d.ws_bytes == (size_t)2 * 24426 * 20);
        CHECK(d.lds_bytes == 64 * 257 * 4 + 64 * 124 && 2 * d.lds_bytes <= 160 * 1024);
        const CspRankPlan s = csp_rank_plan(256, 8142, 64, CSP_IMG_NONE, true);
        CHECK(s.col_parts == 32 && s.n_items == 32 && s.merge_grid == 1);
        CHECK(csp_rank_plan(256, 8142, 100000, CSP_IMG_F64, true).col_parts == 1);
        CHECK(csp_rank_plan(1024, 32768, 1, CSP_IMG_F64, true).lds_bytes <= 160 * 1024);
        CHECK(csp_rank_plan(512, 32768, 1, CSP_IMG_F64, true).lds_bytes <= 160 * 1024);
    }
    check_cover(256, 8142, 24426, CSP_IMG_F32, true, 0, 0, false);
    check_cover(256, 8142, 10000, CSP_IMG_F64, true, 0, 0, false);
    check_cover(256, 8142, 64, CSP_IMG_NONE, true, 0, 0, false);
    check_cover(256, 8142, 24426, CSP_IMG_F32, false, 0, 0, false);
    check_cover(1024, 32768, CSP_HEAD_MAX_B, CSP_IMG_F32, true, 7, 0, false);
    // refusals, each with a reason
    const CspRankPlan bad[] = {
        csp_rank_plan(0, 5, 1, CSP_IMG_F32, true),  csp_rank_plan(1025, 5, 1, CSP_IMG_F32, true),
        csp_rank_plan(256, 0, 1, CSP_IMG_F32, true), csp_rank_plan(256, 32769, 1, CSP_IMG_F32, true),
        csp_rank_plan(256, 5, 0, CSP_IMG_F32, true), csp_rank_plan(256, 5, CSP_HEAD_MAX_B + 1, CSP_IMG_F32, true),
        csp_rank_plan(256, 5, std::numeric_limits<int64_t>::max(), CSP_IMG_F32, true),
        csp_rank_plan(256, 5, 1, -1, true),          csp_rank_plan(256, 5, 1, CSP_IMG_KINDS, true),
        csp_rank_plan(256, 5, 1, CSP_IMG_NONE, false), csp_rank_plan(256, 5, 1, CSP_IMG_F32, true, -1),
        csp_rank_plan(256, 5, 1, CSP_IMG_F32, true, 0, -1), csp_rank_plan(256, 5, 1, CSP_IMG_F32, true, 0, 2),
        csp_rank_plan(256, 8142, 1, CSP_IMG_F32, true, 0, 33)};
    for (const CspRankPlan& p : bad) CHECK(!p.valid && *p.why != 0);
    CHECK(std::strstr(csp_rank_plan(256, 5, 1, CSP_IMG_NONE, false).why, "neither") != nullptr);
    CHECK(std::strstr(csp_rank_plan(256, 8142, 1, CSP_IMG_F32, true, 0, 33).why, "col_parts") != nullptr);
    CHECK(csp_rank_plan(256, 8142, 1, CSP_IMG_F32, true, 0, 32).valid);
    std::printf("csp_rank_plan ok\n");
    return 0;
}
