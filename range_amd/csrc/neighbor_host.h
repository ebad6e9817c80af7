// Host side of the neighbour and grid geo priors (neighbor_kernel.h; include/range_neighbors.h).
// Part of range_hip.hip's translation unit, behind engine_ctx.h.
#pragma once

#include "../../include/range_neighbors.h"

static_assert(RANGE_NEIGHBOR_RADIUS == NEIGHBOR_RADIUS && RANGE_NEIGHBOR_KNN == NEIGHBOR_KNN && RANGE_NEIGHBOR_CELL == NEIGHBOR_CELL &&
              RANGE_NEIGHBOR_MAX_CLASSES == NEIGHBOR_MAX_CLASSES, "host_plan.h and range_neighbors.h disagree");

// ---- the vote scan and the fold (neighbor_kernel.h), by predicate and metric
static void (*neighbor_vote_kernel_for(int mode, bool hav))(NeighborArgs) {
    if (mode == NEIGHBOR_CELL) return neighbor_vote_kernel<NEIGHBOR_CELL, false>;
    if (mode == NEIGHBOR_RADIUS) return hav ? neighbor_vote_kernel<NEIGHBOR_RADIUS, true> : neighbor_vote_kernel<NEIGHBOR_RADIUS, false>;
    return hav ? neighbor_vote_kernel<NEIGHBOR_KNN, true> : neighbor_vote_kernel<NEIGHBOR_KNN, false>;
}
static void (*neighbor_fold_kernel_for(int mode))(NeighborArgs) {
    return mode == NEIGHBOR_CELL ? neighbor_fold_kernel<NEIGHBOR_CELL> : neighbor_fold_kernel<NEIGHBOR_RADIUS>;
}

static int need_neighbors(const range_ctx* c) {
    return c->nb.N ? RANGE_OK : fail(RANGE_ERR_STATE, "no training set installed (range_set_neighbors)");
}

// the classes of a set to install: RANGE_ERR_INVALID names the first outside [0, C)
static int neighbor_check_classes(const int32_t* classes, int64_t N, int32_t C) {
    for (int64_t j = 0; j < N; ++j)
        if (classes[j] < 0 || classes[j] >= C)
            return fail(RANGE_ERR_INVALID, "class %d of training point %lld outside 0 .. %d", classes[j], (long long)j, C - 1);
    return RANGE_OK;
}

// packs N checked points into the context's slot; `extra` (N) int32 or null fills the point's free word: the grid
// cells of range_set_neighbors, or - kde_bits > 0, a weighted set (kde_host.h) - the bins' counts
static int neighbor_install(range_ctx* c, const double* lonlat, const int32_t* classes, const int32_t* extra, int64_t N, int32_t C,
                            int32_t haversine, int kde_bits) {
    ENTER_DEVICE(c);
    HIP_TRY(hipDeviceSynchronize());         // a launch in flight may still read the set this call replaces
    range_ctx::Neighbors& m = c->nb;
    m.N = 0;
    DevBuf<double> d_ll;
    DevBuf<int32_t> d_cls, d_cell;
    HIP_TRY(d_ll.ensure((size_t)N * 2));
    HIP_TRY(d_cls.ensure((size_t)N));
    HIP_TRY(hipMemcpy(d_ll.p, lonlat, (size_t)N * 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_cls.p, classes, (size_t)N * 4, hipMemcpyHostToDevice));
    if (extra) {
        HIP_TRY(d_cell.ensure((size_t)N));
        HIP_TRY(hipMemcpy(d_cell.p, extra, (size_t)N * 4, hipMemcpyHostToDevice));
    }
    HIP_TRY(m.d_pts.ensure((size_t)N));
    const int64_t n_tiles = (N + NEIGHBOR_BLOCK - 1) / NEIGHBOR_BLOCK;
    const unsigned grid = (unsigned)std::min<int64_t>(n_tiles, NEIGHBOR_MAX_GRID);
    if (int rc = launch(neighbor_prep_kernel, dim3(grid), dim3(NEIGHBOR_BLOCK), 0, (hipStream_t) nullptr, (const double*)d_ll.p,
                        (const int32_t*)d_cls.p, (const int32_t*)d_cell.p, N, (int32_t)(haversine != 0), m.d_pts.p))
        return rc;
    HIP_TRY(hipDeviceSynchronize());
    m.C = C;
    m.hav = haversine != 0;
    m.has_cells = extra != nullptr && kde_bits == 0;
    m.kde_bits = kde_bits;
    m.N = N;
    return RANGE_OK;
}

static int neighbor_select_impl(range_ctx* c, const double* q, int64_t B, int64_t k, double* red_k, int64_t* j_last,
                                int64_t max_grid, hipStream_t s) {
    if (k < 1 || k > c->nb.N)
        return fail(RANGE_ERR_INVALID, "k = %lld neighbours of %lld training points (1 .. N)", (long long)k, (long long)c->nb.N);
    const NeighborPlan p = neighbor_plan(B, c->nb.N, c->nb.C, k, max_grid, 0);
    if (!p.valid) return fail(RANGE_ERR_INVALID, "B = %lld: %s", (long long)B, p.why);
    NeighborSelectArgs a{};
    a.pts = c->nb.d_pts.p;
    a.N = c->nb.N;
    a.q = q;
    a.B = B;
    a.k = k;
    a.red_k = red_k;
    a.j_last = j_last;
    return launch(c->nb.hav ? neighbor_select_kernel<true> : neighbor_select_kernel<false>, dim3(p.select_grid), dim3(p.block), 0, s, a);
}

// ---- what the scans of both row kinds share (neighbor_run here, kde_run in kde_host.h)

// the checks of the common arguments; own: the caller's refusal of an argument of its own (or null), at its place
// in the order; own_aligned: the caller's own device pointers are aligned to their element
static int neighbor_check_scan(int64_t B, int64_t max_grid, int32_t chunks, const char* own, const void* img, int32_t img_kind,
                               const int32_t* labels, const int32_t* greater, const int32_t* tied, const int32_t* argmax,
                               const double* prior, bool own_aligned) {
    if (B <= 0) return fail(RANGE_ERR_INVALID, "B must be > 0");
    if (max_grid < 0 || chunks < 0) return fail(RANGE_ERR_INVALID, "max_grid and chunks must be >= 0");
    if (own) return fail(RANGE_ERR_INVALID, "%s", own);
    if (greater) {
        if (!labels || !tied || !argmax) return fail(RANGE_ERR_INVALID, "null argument");
        if (int rc = check_img_kind(img, img_kind)) return rc;
    }
    if (!own_aligned || !aligned(labels, 4) || !aligned(greater, 4) || !aligned(tied, 4) || !aligned(argmax, 4) || !aligned(prior, 8) ||
        !aligned(img, img_kind == CSP_IMG_F64 ? 8 : 4))
        return fail(RANGE_ERR_INVALID, "the device pointers must be aligned to their element");
    return RANGE_OK;
}

// the common part of a scan's arguments from the installed set and the plan
static void neighbor_fill_scan(NeighborScanArgs& a, const range_ctx::Neighbors& m, const NeighborPlan& p, const double* q, int64_t B,
                               const void* img, int32_t img_kind, const int32_t* labels, int32_t* greater, int32_t* tied,
                               int32_t* argmax, double* prior) {
    a.pts = m.d_pts.p;
    a.N = m.N;
    a.n_tiles = p.n_tiles;
    a.q = q;
    a.B = B;
    a.groups = p.groups;
    a.G = p.group;
    a.C = m.C;
    a.img = greater ? img : nullptr;
    a.img_kind = greater ? img_kind : CSP_IMG_NONE;
    a.labels = labels;
    a.greater = greater;
    a.tied = tied;
    a.argmax = argmax;
    a.prior = prior;
    a.chunks = p.chunks;
}

// the vote launch over (groups, chunks) and, with more than one chunk, the workspace before it and the fold behind it
template <class Args>
static int neighbor_launch_scan(range_ctx* c, const NeighborPlan& p, void (*vote)(Args), void (*fold)(Args), Args& a, hipStream_t s) {
    if (p.chunks > 1) {
        if (c->nb.ws_rows.ensure((p.ws_bytes + 7) / 8) != hipSuccess)
            return fail(RANGE_ERR_NOMEM, "out of device memory (%zu bytes of partial rows)", p.ws_bytes);
        a.ws = reinterpret_cast<decltype(a.ws)>(c->nb.ws_rows.p);
    }
    if (int rc = launch(vote, dim3(p.grid, (unsigned)p.chunks), dim3(p.vote_block), p.lds_bytes, s, a)) return rc;
    if (p.chunks == 1) return RANGE_OK;
    return launch(fold, dim3(p.fold_grid), dim3(p.vote_block), p.lds_bytes, s, a);
}

// the vote scan (and the fold) of B queries into whichever outputs are given
static int neighbor_run(range_ctx* c, const double* q, const int32_t* qcell, int64_t B, int32_t mode, int64_t k, double thr,
                        double pc, double cpc, const void* img, int32_t img_kind, const int32_t* labels, int32_t* greater,
                        int32_t* tied, int32_t* argmax, double* prior, int32_t* counts, int64_t max_grid, int32_t chunks,
                        range_stream_t stream) {
    if (!c) return fail(RANGE_ERR_INVALID, "null argument");
    if (int rc = need_neighbors(c)) return rc;
    if (mode < 0 || mode >= NEIGHBOR_MODES) return fail(RANGE_ERR_INVALID, "mode %d", mode);
    if (mode == NEIGHBOR_CELL ? (!qcell || !c->nb.has_cells) : !q)
        return fail(RANGE_ERR_INVALID, mode == NEIGHBOR_CELL ? "the cell predicate needs qcell and a training set installed with cells"
                                                             : "null queries");
    if (int rc = neighbor_check_scan(B, max_grid, chunks, mode == NEIGHBOR_RADIUS && thr != thr ? "the threshold is NaN" : nullptr, img,
                                     img_kind, labels, greater, tied, argmax, prior,
                                     aligned(q, 8) && aligned(qcell, 4) && aligned(counts, 4)))
        return rc;
    range_ctx::Neighbors& m = c->nb;
    const NeighborPlan p = neighbor_plan(B, m.N, m.C, mode == NEIGHBOR_KNN ? k : 0, max_grid, chunks);
    if (!p.valid) return fail(RANGE_ERR_INVALID, "B = %lld, k = %lld: %s", (long long)B, (long long)k, p.why);
    ENTER_DEVICE(c);
    const hipStream_t s = (hipStream_t)stream;
    NeighborArgs a{};
    neighbor_fill_scan(a, m, p, q, B, img, img_kind, labels, greater, tied, argmax, prior);
    a.qcell = qcell;
    a.thr = thr;
    a.pc = pc;
    a.cpc = cpc;
    a.raw = counts;
    if (mode == NEIGHBOR_KNN) {
        if (m.ws_redk.ensure((size_t)B) != hipSuccess || m.ws_jlast.ensure((size_t)B) != hipSuccess)
            return fail(RANGE_ERR_NOMEM, "out of device memory (%lld selections)", (long long)B);
        if (int rc = neighbor_select_impl(c, q, B, k, m.ws_redk.p, m.ws_jlast.p, max_grid, s)) return rc;
        a.red_k = m.ws_redk.p;
        a.j_last = m.ws_jlast.p;
    }
    return neighbor_launch_scan(c, p, neighbor_vote_kernel_for(mode, m.hav), neighbor_fold_kernel_for(mode), a, s);
}

// the six leading slots of range_neighbor_plan's and range_kde_plan's out[]
static void neighbor_plan_out(const NeighborPlan& p, int64_t* out) {
    out[0] = p.group;
    out[1] = p.groups;
    out[2] = p.grid;
    out[3] = p.chunks;
    out[4] = (int64_t)p.lds_bytes;
    out[5] = (int64_t)p.ws_bytes;
}

extern "C" {

int range_neighbor_plan(int64_t B, int64_t N, int32_t C, int64_t k, int64_t max_grid, int32_t chunks, int64_t* out) {
    if (!out) return fail(RANGE_ERR_INVALID, "null argument");
    const NeighborPlan p = neighbor_plan(B, N, C, k, max_grid, chunks);
    if (!p.valid) return fail(RANGE_ERR_INVALID, "B = %lld, N = %lld, C = %d, k = %lld: %s", (long long)B, (long long)N, C, (long long)k, p.why);
    neighbor_plan_out(p, out);
    out[6] = NEIGHBOR_DIGIT_BITS;
    out[7] = NEIGHBOR_PASSES;
    return RANGE_OK;
}

int range_set_neighbors(range_ctx* c, const double* lonlat, const int32_t* classes, const int32_t* cells, int64_t N, int32_t C,
                        int32_t haversine) {
    if (!c || !lonlat || !classes) return fail(RANGE_ERR_INVALID, "null argument");
    const NeighborPlan p = neighbor_plan(1, N, C, 0);
    if (!p.valid) return fail(RANGE_ERR_INVALID, "N = %lld, C = %d: %s", (long long)N, C, p.why);
    if (int rc = neighbor_check_classes(classes, N, C)) return rc;
    return neighbor_install(c, lonlat, classes, cells, N, C, haversine, 0);
}

int64_t range_neighbor_points(const range_ctx* c) { return c ? c->nb.N : 0; }
int32_t range_neighbor_classes(const range_ctx* c) { return c && c->nb.N ? c->nb.C : 0; }

int range_neighbor_select_grid(range_ctx* c, const double* q, int64_t B, int64_t k, double* red_k, int64_t* j_last, int64_t max_grid,
                               range_stream_t stream) {
    if (!c || !q || !red_k || !j_last) return fail(RANGE_ERR_INVALID, "null argument");
    if (int rc = need_neighbors(c)) return rc;
    if (B <= 0) return fail(RANGE_ERR_INVALID, "B must be > 0");
    if (max_grid < 0) return fail(RANGE_ERR_INVALID, "max_grid must be >= 0");
    if (!aligned(q, 8) || !aligned(red_k, 8) || !aligned(j_last, 8)) return fail(RANGE_ERR_INVALID, "the device pointers must be 8-byte aligned");
    ENTER_DEVICE(c);
    return neighbor_select_impl(c, q, B, k, red_k, j_last, max_grid, (hipStream_t)stream);
}

int range_neighbor_select(range_ctx* c, const double* q, int64_t B, int64_t k, double* red_k, int64_t* j_last, range_stream_t stream) {
    return range_neighbor_select_grid(c, q, B, k, red_k, j_last, 0, stream);
}

int range_neighbor_rank_grid(range_ctx* c, const double* q, const int32_t* qcell, int64_t B, int32_t mode, int64_t k, double thr,
                             double pc, double cpc, const void* img, int32_t img_kind, const int32_t* labels, int32_t* greater,
                             int32_t* tied_after, int32_t* argmax, int64_t max_grid, int32_t chunks, range_stream_t stream) {
    if (!labels || !greater || !tied_after || !argmax) return fail(RANGE_ERR_INVALID, "null argument");
    return neighbor_run(c, q, qcell, B, mode, k, thr, pc, cpc, img, img_kind, labels, greater, tied_after, argmax, nullptr, nullptr,
                        max_grid, chunks, stream);
}

int range_neighbor_rank(range_ctx* c, const double* q, const int32_t* qcell, int64_t B, int32_t mode, int64_t k, double thr, double pc,
                        double cpc, const void* img, int32_t img_kind, const int32_t* labels, int32_t* greater, int32_t* tied_after,
                        int32_t* argmax, range_stream_t stream) {
    return range_neighbor_rank_grid(c, q, qcell, B, mode, k, thr, pc, cpc, img, img_kind, labels, greater, tied_after, argmax, 0, 0, stream);
}

int range_neighbor_prior_grid(range_ctx* c, const double* q, const int32_t* qcell, int64_t B, int32_t mode, int64_t k, double thr,
                              double pc, double cpc, double* prior, int32_t* counts, int64_t max_grid, int32_t chunks,
                              range_stream_t stream) {
    if (!prior && !counts) return fail(RANGE_ERR_INVALID, "null argument");
    return neighbor_run(c, q, qcell, B, mode, k, thr, pc, cpc, nullptr, CSP_IMG_NONE, nullptr, nullptr, nullptr, nullptr, prior, counts,
                        max_grid, chunks, stream);
}

int range_neighbor_prior(range_ctx* c, const double* q, const int32_t* qcell, int64_t B, int32_t mode, int64_t k, double thr, double pc,
                         double cpc, double* prior, range_stream_t stream) {
    if (!prior) return fail(RANGE_ERR_INVALID, "null argument");
    return range_neighbor_prior_grid(c, q, qcell, B, mode, k, thr, pc, cpc, prior, nullptr, 0, 0, stream);
}

}  // extern "C"
