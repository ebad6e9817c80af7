// Host side of the KDE geo prior (kde_kernel.h; include/range_neighbors.h).
// Part of range_hip.hip's translation unit, behind neighbor_host.h.
#pragma once

#include <cmath>

static_assert(RANGE_KDE_MAX_CLASSES == KDE_MAX_CLASSES, "host_plan.h and range_neighbors.h disagree");

static int need_kde_points(const range_ctx* c) {
    if (int rc = need_neighbors(c)) return rc;
    return c->nb.kde_bits ? RANGE_OK
                          : fail(RANGE_ERR_STATE, "the installed set has no counts: the KDE calls need range_set_kde_points, not range_set_neighbors");
}

// the KDE scan (and the fold) of B queries into whichever outputs are given
static int kde_run(range_ctx* c, const double* q, const double* thr, const double* two_h2, int64_t B, const void* img, int32_t img_kind,
                   const int32_t* labels, int32_t* greater, int32_t* tied, int32_t* argmax, double* prior, uint64_t* sums,
                   int64_t max_grid, int32_t chunks, range_stream_t stream) {
    if (!c || !q || !thr || !two_h2) return fail(RANGE_ERR_INVALID, "null argument");
    if (int rc = need_kde_points(c)) return rc;
    if (int rc = neighbor_check_scan(B, max_grid, chunks, nullptr, img, img_kind, labels, greater, tied, argmax, prior,
                                     aligned(q, 8) && aligned(thr, 8) && aligned(two_h2, 8) && aligned(sums, 8)))
        return rc;
    range_ctx::Neighbors& m = c->nb;
    // (the total count enters the plan through the scale bits alone, which the installation fixed)
    const KdePlan p = kde_plan(B, m.N, m.C, m.N, max_grid, chunks);
    if (!p.valid) return fail(RANGE_ERR_INVALID, "B = %lld: %s", (long long)B, p.why);
    ENTER_DEVICE(c);
    KdeArgs a{};
    neighbor_fill_scan(a, m, p, q, B, img, img_kind, labels, greater, tied, argmax, prior);
    a.thr = thr;
    a.two_h2 = two_h2;
    a.scale = std::ldexp(1.0, m.kde_bits);
    a.raw = sums;
    return neighbor_launch_scan(c, p, m.hav ? kde_vote_kernel<true> : kde_vote_kernel<false>, kde_fold_kernel, a, (hipStream_t)stream);
}

extern "C" {

int range_kde_plan(int64_t B, int64_t M, int32_t C, int64_t total_count, int64_t max_grid, int32_t chunks, int64_t* out) {
    if (!out) return fail(RANGE_ERR_INVALID, "null argument");
    const KdePlan p = kde_plan(B, M, C, total_count, max_grid, chunks);
    if (!p.valid)
        return fail(RANGE_ERR_INVALID, "B = %lld, M = %lld, C = %d, total count %lld: %s", (long long)B, (long long)M, C, (long long)total_count, p.why);
    neighbor_plan_out(p, out);
    out[6] = p.scale_bits;
    out[7] = p.n_tiles;
    return RANGE_OK;
}

int range_set_kde_points(range_ctx* c, const double* lonlat, const int32_t* classes, const int32_t* counts, int64_t M, int32_t C,
                         int32_t haversine) {
    if (!c || !lonlat || !classes || !counts) return fail(RANGE_ERR_INVALID, "null argument");
    if (M < 1 || M > NEIGHBOR_MAX_POINTS) return fail(RANGE_ERR_INVALID, "M = %lld outside 1 .. 2^31 - 1", (long long)M);
    int64_t total = 0;
    for (int64_t j = 0; j < M; ++j) {
        if (counts[j] < 1) return fail(RANGE_ERR_INVALID, "count %d of bin %lld: must be >= 1", counts[j], (long long)j);
        total += counts[j];
        if (total > KDE_MAX_TOTAL) return fail(RANGE_ERR_INVALID, "the counts up to bin %lld sum beyond 2^31 - 1", (long long)j);
    }
    const KdePlan p = kde_plan(1, M, C, total);
    if (!p.valid) return fail(RANGE_ERR_INVALID, "M = %lld, C = %d: %s", (long long)M, C, p.why);
    if (int rc = neighbor_check_classes(classes, M, C)) return rc;
    return neighbor_install(c, lonlat, classes, counts, M, C, haversine, p.scale_bits);
}

int32_t range_kde_scale_bits(const range_ctx* c) { return c && c->nb.N ? c->nb.kde_bits : 0; }

int range_kde_rank_grid(range_ctx* c, const double* q, const double* thr, const double* two_h2, int64_t B, const void* img,
                        int32_t img_kind, const int32_t* labels, int32_t* greater, int32_t* tied_after, int32_t* argmax,
                        int64_t max_grid, int32_t chunks, range_stream_t stream) {
    if (!labels || !greater || !tied_after || !argmax) return fail(RANGE_ERR_INVALID, "null argument");
    return kde_run(c, q, thr, two_h2, B, img, img_kind, labels, greater, tied_after, argmax, nullptr, nullptr, max_grid, chunks, stream);
}

int range_kde_rank(range_ctx* c, const double* q, const double* thr, const double* two_h2, int64_t B, const void* img, int32_t img_kind,
                   const int32_t* labels, int32_t* greater, int32_t* tied_after, int32_t* argmax, range_stream_t stream) {
    return range_kde_rank_grid(c, q, thr, two_h2, B, img, img_kind, labels, greater, tied_after, argmax, 0, 0, stream);
}

int range_kde_prior_grid(range_ctx* c, const double* q, const double* thr, const double* two_h2, int64_t B, double* prior,
                         uint64_t* sums, int64_t max_grid, int32_t chunks, range_stream_t stream) {
    if (!prior && !sums) return fail(RANGE_ERR_INVALID, "null argument");
    return kde_run(c, q, thr, two_h2, B, nullptr, CSP_IMG_NONE, nullptr, nullptr, nullptr, nullptr, prior, sums, max_grid, chunks, stream);
}

int range_kde_prior(range_ctx* c, const double* q, const double* thr, const double* two_h2, int64_t B, double* prior,
                    range_stream_t stream) {
    if (!prior) return fail(RANGE_ERR_INVALID, "null argument");
    return range_kde_prior_grid(c, q, thr, two_h2, B, prior, nullptr, 0, 0, stream);
}

}  // extern "C"
