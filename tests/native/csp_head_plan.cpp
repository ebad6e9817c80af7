// The launch plan and the packing of the CSP class head (range_amd/csrc/host_plan.h: csp_head_plan,
// csp_pack_head) on the CPU, built with g++ under AddressSanitizer / UndefinedBehaviorSanitizer by
// tests/test_csp_head_cpu.py.  At the corners of the envelope: every class_emb (n, k) lands exactly once in the
// packed image, where the kernel's lane reads it (csp_head_kernel.h), the padding is zero; every index the kernel
// forms stays inside the LDS image and the packed image; the work items of a launch - walked grid-stride by
// the workgroups, every wave its column tiles - cover B x M exactly once, also with a capped grid; the refusals;
// the rows of a chunk of the composed calls (csp_predict_chunk) at every width.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../range_amd/csrc/host_plan.h"

using namespace range_host;

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); std::exit(1); } \
    } while (0)

static void check_packing(int K, int C) {
    const CspHeadPlan p = csp_head_plan(K, C, C, 1, CSP_HEAD_PROBS);
    CHECK(p.valid && p.num_filts == K && p.num_classes == C && p.M == C);
    CHECK(p.m_tiles == (K <= 512 ? 2 : 1) && p.tile_rows == 32 * p.m_tiles && p.block == CSP_BLOCK);
    CHECK(p.k_groups * CSP_KGROUP >= K && p.k_groups * CSP_KGROUP - K < CSP_KGROUP);
    CHECK(p.n_tiles * CSP_NTILE >= C && p.n_tiles * CSP_NTILE - C < CSP_NTILE);
    CHECK(p.ld % 2 == 1 && p.ld > p.k_groups * CSP_KGROUP);
    CHECK(p.lds_bytes == ((size_t)p.tile_rows * p.ld + 4 * (size_t)p.tile_rows) * 4 && p.lds_bytes <= 160 * 1024);
    CHECK(p.wave_tiles * p.m_tiles == CSP_HEAD_ACC_TILES && p.cols_per_pass == 4 * p.wave_tiles * 32);
    CHECK(p.packed_floats == (size_t)p.n_tiles * 32 * p.k_groups * 8 && p.packed_floats / 4 < (size_t)1 << 32);
    // the A operand's last read of a row: column k_pad - 2 + 1 of row T - 1 (csp_head_gemm: xa[m * 32 ld + 8 kg + 2 s])
    CHECK((size_t)(p.tile_rows - 1) * p.ld + 1 + (size_t)p.k_groups * 8 - 2 < (size_t)p.tile_rows * p.ld);
    std::vector<float> w((size_t)C * K), packed(p.packed_floats, 0.0f);
    for (size_t j = 0; j < w.size(); ++j) w[j] = (float)(1 + j % 16000000);
    csp_pack_head(p, w.data(), packed.data());
    const CspLayerPlan l = p.layer();
    size_t nonzero = 0;
    // the kernel's read: lane (class id, k parity lh) takes float4 ((id >> 5) k_groups + kg) 64 + 32 lh + (id & 31),
    // component s of it is k = 8 kg + 2 s + lh
    for (int id = 0; id < p.n_tiles * 32; ++id)
        for (int kg = 0; kg < p.k_groups; ++kg)
            for (int lh = 0; lh < 2; ++lh)
                for (int s = 0; s < 4; ++s) {
                    const size_t f4 = ((size_t)(id >> 5) * p.k_groups + kg) * 64 + 32 * lh + (id & 31);
                    const size_t at = f4 * 4 + s;
                    CHECK(at < p.packed_floats);
                    const int k = kg * 8 + 2 * s + lh;
                    const float want = id < C && k < K ? w[(size_t)id * K + k] : 0.0f;     // the padding is zero
                    CHECK(packed[at] == want);
                    if (id < C && k < K) { CHECK(at == csp_packed_index(l, id, k)); ++nonzero; }
                }
    CHECK(nonzero == w.size());
}

// every (row, column) of B x M exactly once: rows by row tile, columns by the waves' tiles of the items' chunks
static void check_cover(int K, int C, int64_t M, int64_t B, int mode, int64_t cap, bool count_cells) {
    const CspHeadPlan p = csp_head_plan(K, C, M, B, mode, cap);
    CHECK(p.valid && p.grid >= 1 && (int64_t)p.grid <= CSP_MAX_GRID && (int64_t)p.grid <= p.n_items);
    if (cap) CHECK((int64_t)p.grid <= cap);
    CHECK(p.row_tiles * p.tile_rows >= B && (p.row_tiles - 1) * p.tile_rows < B);
    CHECK((int64_t)p.n_chunks * p.cols_per_pass >= M && (int64_t)(p.n_chunks - 1) * p.cols_per_pass < M);
    CHECK((int64_t)p.col_tiles * 32 >= M && (int64_t)(p.col_tiles - 1) * 32 < M);
    CHECK(p.chunks_per_item >= 1 && p.groups == (p.n_chunks + p.chunks_per_item - 1) / p.chunks_per_item);
    if (mode == CSP_HEAD_SUM) CHECK(p.chunks_per_item == p.n_chunks && p.groups == 1);
    else CHECK(p.chunks_per_item == 1 || (p.chunks_per_item <= 8 && p.row_tiles * p.groups >= CSP_MAX_GRID));
    CHECK(p.n_items == p.row_tiles * p.groups);
    int64_t sum = 0;
    for (int64_t blk = 0; blk < (int64_t)p.grid; ++blk) sum += p.items_of(blk);
    CHECK(sum == p.n_items && p.items_of(p.n_items) == 0);
    if (!count_cells) return;
    std::vector<unsigned char> hit((size_t)B * (size_t)M, 0);
    for (int64_t blk = 0; blk < (int64_t)p.grid; ++blk)
        for (int64_t it = blk; it < p.n_items; it += p.grid) {
            int64_t rt;
            int ch0, ch1;
            p.item(it, rt, ch0, ch1);
            CHECK(rt >= 0 && rt < p.row_tiles && ch0 >= 0 && ch0 < ch1 && ch1 <= p.n_chunks);
            for (int ch = ch0; ch < ch1; ++ch)
                for (int w = 0; w < 4; ++w) {
                    const int n = p.wave_n_tiles(ch, w);
                    CHECK(n >= 0 && n <= p.wave_tiles);
                    for (int j = 0; j < n; ++j) {
                        const int tile = p.wave_first_tile(ch, w) + 4 * j;
                        CHECK(tile < p.col_tiles);
                        for (int c = tile * 32; c < tile * 32 + 32 && c < M; ++c)
                            for (int64_t r = rt * p.tile_rows; r < (rt + 1) * p.tile_rows && r < B; ++r) {
                                CHECK(hit[(size_t)r * M + c] == 0);
                                hit[(size_t)r * M + c] = 1;
                            }
                    }
                }
        }
    for (unsigned char h : hit) CHECK(h == 1);
}

int main() {
    // the envelope's corners of the packing: num_filts 1, 8, 9, 24, 50, 256, 512, 513, 600, 1024; classes 1, 31 .. 33, the
    // design head, 32768 (with a narrow net: the widest image, 32768 x 1024, is 128 MiB and only planned)
    for (int K : {1, 8, 9, 24, 50, 256, 512, 513, 600, 1024})
        for (int C : {1, 5, 31, 32, 33, 1025}) check_packing(K, C);
    check_packing(256, 8142);
    check_packing(24, 32768);
    {
        const CspHeadPlan p = csp_head_plan(1024, 32768, 32768, 1, CSP_HEAD_PROBS);
        CHECK(p.valid && p.packed_floats == (size_t)32768 * 1024 && p.tile_rows == 32 && p.cols_per_pass == 512);
        const CspHeadPlan d = csp_head_plan(256, 8142, 8142, 10000, CSP_HEAD_PROBS);
        CHECK(d.tile_rows == 64 && d.ld == 257 && d.cols_per_pass == 256 && d.n_chunks == 32 && d.row_tiles == 157);
        CHECK(d.chunks_per_item == 2 && d.groups == 16 && d.n_items == 157 * 16 && d.grid == 2048);
        CHECK(d.lds_bytes == (64 * 257 + 256) * 4 && 2 * d.lds_bytes <= 160 * 1024);      // two workgroups a CU
        const CspHeadPlan big = csp_head_plan(256, 8142, 8142, 100000, CSP_HEAD_PROBS);
        CHECK(big.chunks_per_item == 8 && big.groups == 4 && big.n_items == 1563 * 4);
        CHECK(csp_head_plan(256, 8142, 8142, 64, CSP_HEAD_PROBS).chunks_per_item == 1);
    }
    for (int K : {24, 600})
        for (int mode : {CSP_HEAD_PROBS, CSP_HEAD_LOGITS, CSP_HEAD_SUM}) {
            const int P = csp_head_plan(K, 1, 1, 1, CSP_HEAD_PROBS).cols_per_pass;
            for (int C : {1, 31, 32, 33, P - 1, P, P + 1, 2 * P + 1})
                for (int64_t B : {INT64_C(1), INT64_C(31), INT64_C(33), INT64_C(63), INT64_C(64), INT64_C(65), INT64_C(129)})
                    for (int64_t cap : {INT64_C(0), INT64_C(1), INT64_C(3)}) check_cover(K, C, C, B, mode, cap, true);
        }
    // a subset: M ids of C classes, M beyond C (repeats) too
    for (int64_t M : {INT64_C(1), INT64_C(33), INT64_C(700)}) check_cover(256, 40, M, 70, CSP_HEAD_PROBS, 0, true);
    // large launches: the item counts only
    check_cover(256, 8142, 8142, 10000, CSP_HEAD_PROBS, 0, false);
    check_cover(256, 8142, 1, 2000000, CSP_HEAD_PROBS, 0, false);
    check_cover(256, 8142, 8142, 100000, CSP_HEAD_SUM, 0, false);
    check_cover(1024, 32768, 32768, CSP_HEAD_MAX_B, CSP_HEAD_LOGITS, 0, false);
    check_cover(256, 32768, CSP_HEAD_MAX_M, (INT64_C(1) << 31) + 5, CSP_HEAD_PROBS, 7, false);
    // refusals
    CHECK(!csp_head_plan(0, 5, 5, 1, 0).valid && !csp_head_plan(1025, 5, 5, 1, 0).valid);
    CHECK(!csp_head_plan(256, 0, 1, 1, 0).valid && !csp_head_plan(256, 32769, 32769, 1, 0).valid);
    CHECK(!csp_head_plan(256, 5, 0, 1, 0).valid && !csp_head_plan(256, 5, (int64_t)CSP_HEAD_MAX_M + 1, 1, 0).valid);
    CHECK(!csp_head_plan(256, 5, 5, 0, 0).valid && !csp_head_plan(256, 5, 5, CSP_HEAD_MAX_B + 1, 0).valid);
    CHECK(!csp_head_plan(256, 5, 5, std::numeric_limits<int64_t>::max(), 0).valid);
    CHECK(!csp_head_plan(256, 5, 5, 1, -1).valid && !csp_head_plan(256, 5, 5, 1, CSP_HEAD_MODES).valid);
    CHECK(!csp_head_plan(256, 5, 5, 1, 0, -1).valid);
    CHECK(!csp_head_plan(256, 5, 3, 1, CSP_HEAD_SUM).valid && csp_head_plan(256, 5, 5, 1, CSP_HEAD_SUM).valid);
    CHECK(*csp_head_plan(256, 32769, 1, 1, 0).why != 0);
    // a chunk of the composed calls: whole 64-row tiles, at most 2^16 rows and 64 MiB of float32 embeddings
    for (int width = 1; width <= CSP_MAX_WIDTH; ++width) {
        const int64_t chunk = csp_predict_chunk(width);
        CHECK(chunk > 0 && chunk % 64 == 0 && chunk <= 65536 && chunk * width * 4 <= (INT64_C(64) << 20));
        CHECK(chunk == std::min<int64_t>(INT64_C(1) << 16, (INT64_C(1) << 24) / width / 64 * 64));
    }
    for (int width : {256, 257, 1024}) std::printf("csp_predict_chunk(%d) = %lld\n", width, (long long)csp_predict_chunk(width));
    std::printf("csp_head_plan ok\n");
    return 0;
}
