/* range_neighbors.h - C ABI of the neighbour and grid geo priors in librange_hip.so (MI355X / gfx950).
 *
 * Replaces the per-sample BallTree queries and dense priors of the reference's location-only baselines
 * (location_models/csp/main/baselines.py: compute_neighbor_prior - 'nn_dist', 'nn_knn' - and GridPrior -
 * 'grid'; eval_helper.py: compute_acc_batch).  A training set (locations, classes, optional grid cells) is
 * installed on a range_ctx once; queries are then scanned against it (csrc/neighbor_kernel.h).
 *
 * Conventions: as range_hip.h.  Locations are (lon, lat) float64 pairs: RADIANS when the set was installed
 * with haversine = 1, else DEGREES.  The reduced distance red(i, j) of query i and training point j is
 *   haversine: sin(.5 (lat_i - lat_j))^2 + cos(lat_i) cos(lat_j) sin(.5 (lon_i - lon_j)) sin(.5 (lon_i - lon_j))
 *   euclidean: (lat_i - lat_j)^2 + (lon_i - lon_j)^2
 * in float64, scikit-learn's expression order, nothing contracted.  A training point j votes for its class in
 * the row of query i when (mode)
 *   RANGE_NEIGHBOR_RADIUS: red(i, j) <= thr;
 *   RANGE_NEIGHBOR_KNN:    (red(i, j), j) is among the k smallest pairs of the row under the total order
 *                          (red, then j).  BallTree leaves the choice among equal distances unspecified; this
 *                          order is the rule here;
 *   RANGE_NEIGHBOR_CELL:   qcell[i] == cell[j] (qcell -1: the uniform prior; a training cell < 0 never votes).
 * A NaN red is never a member.  With cnt[c] the votes of a row, n their sum and C the classes
 *   RADIUS / KNN: prior[c] = (1.0 + cnt[c]) / (double)(C + n)
 *   CELL:         prior[c] = ((cnt[c] + pc) - 1.0) / ((n + cpc) - C), 1.0 / C for qcell -1  (cpc: C * pc from the caller)
 * and the score is (double) img[c] * prior[c], or prior[c] with RANGE_CSP_IMG_NONE.  greater / tied_after /
 * argmax and their -1 (the label's score is NaN) / -2 (label outside [0, C)) flags: as range_csp_rank.
 * No result depends on the launch geometry (max_grid, chunks), the stream or earlier calls, bit for bit.
 */
#ifndef RANGE_NEIGHBORS_H
#define RANGE_NEIGHBORS_H

#include "range_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RANGE_NEIGHBOR_RADIUS 0
#define RANGE_NEIGHBOR_KNN 1
#define RANGE_NEIGHBOR_CELL 2
#define RANGE_NEIGHBOR_MAX_CLASSES 32768 /* one int32 count row of a query must fit the CU's LDS */

/* The launch plan (a pure function of its arguments, no device): out[0] = queries of a workgroup (G),
 * [1] = query groups, [2] = workgroups over the groups, [3] = chunks of the training set, [4] = LDS bytes,
 * [5] = workspace bytes of the partial counts (0 with one chunk), [6] = bits of a selection digit,
 * [7] = passes of the selection.  k = 0: no selection.  RANGE_ERR_INVALID: B or N outside 1 .. 2^31 - 1,
 * C outside 1 .. RANGE_NEIGHBOR_MAX_CLASSES, k > N, a negative argument. */
int range_neighbor_plan(int64_t B, int64_t N, int32_t C, int64_t k, int64_t max_grid, int32_t chunks,
                        int64_t* out8_host);

/* Installs N training points: lonlat_host (N, 2), classes_host (N) in [0, C), cells_host (N) int32 or NULL
 * (no RANGE_NEIGHBOR_CELL calls then).  Packs them on the device with cos(lat) formed once (haversine).
 * Host arrays, read during the call; synchronous; replaces an earlier set.  RANGE_ERR_INVALID names the
 * first class outside [0, C). */
int range_set_neighbors(range_ctx* ctx, const double* lonlat_host, const int32_t* classes_host,
                        const int32_t* cells_host, int64_t N, int32_t C, int32_t haversine);
int64_t range_neighbor_points(const range_ctx* ctx);
int32_t range_neighbor_classes(const range_ctx* ctx);

/* Per query the k-th smallest pair (red, j): red_k_dev (B) float64 and j_last_dev (B) int64, the index of the
 * last pair taken among those whose red equals red_k.  A query with fewer than k pairs whose red is a number
 * (a NaN query): red_k NaN, j_last -1.  RANGE_ERR_INVALID: k outside 1 .. N (BallTree.query refuses k > N). */
int range_neighbor_select(range_ctx* ctx, const double* q_dev, int64_t B, int64_t k, double* red_k_dev,
                          int64_t* j_last_dev, range_stream_t stream);
int range_neighbor_select_grid(range_ctx* ctx, const double* q_dev, int64_t B, int64_t k, double* red_k_dev,
                               int64_t* j_last_dev, int64_t max_grid, range_stream_t stream);

/* The three rank integers of B queries.  q_dev (B, 2), NULL with RANGE_NEIGHBOR_CELL; qcell_dev (B) int32,
 * RANGE_NEIGHBOR_CELL only.  mode RADIUS reads thr, KNN reads k (the selection runs inside the call), CELL
 * reads pc and cpc.  img_dev (B, C) of img_kind (RANGE_CSP_IMG_*) or NULL; labels_dev (B) int32. */
int range_neighbor_rank(range_ctx* ctx, const double* q_dev, const int32_t* qcell_dev, int64_t B, int32_t mode,
                        int64_t k, double thr, double pc, double cpc, const void* img_dev, int32_t img_kind,
                        const int32_t* labels_dev, int32_t* greater_dev, int32_t* tied_after_dev,
                        int32_t* argmax_dev, range_stream_t stream);
int range_neighbor_rank_grid(range_ctx* ctx, const double* q_dev, const int32_t* qcell_dev, int64_t B, int32_t mode,
                             int64_t k, double thr, double pc, double cpc, const void* img_dev, int32_t img_kind,
                             const int32_t* labels_dev, int32_t* greater_dev, int32_t* tied_after_dev,
                             int32_t* argmax_dev, int64_t max_grid, int32_t chunks, range_stream_t stream);

/* The (B, C) float64 priors of B queries; the _grid form also gives the (B, C) int32 votes (counts_dev, or
 * NULL) and may leave prior_dev NULL. */
int range_neighbor_prior(range_ctx* ctx, const double* q_dev, const int32_t* qcell_dev, int64_t B, int32_t mode,
                         int64_t k, double thr, double pc, double cpc, double* prior_dev, range_stream_t stream);
int range_neighbor_prior_grid(range_ctx* ctx, const double* q_dev, const int32_t* qcell_dev, int64_t B, int32_t mode,
                              int64_t k, double thr, double pc, double cpc, double* prior_dev, int32_t* counts_dev,
                              int64_t max_grid, int32_t chunks, range_stream_t stream);

/* ---- The KDE prior ('kde': baselines.py create_kde_grid / kde_prior; csrc/kde_kernel.h).
 *
 * A WEIGHTED set of M bins (class, location, count >= 1) takes the context's neighbour slot.  Per query i the caller
 * gives thr[i] and two_h2[i] (float64; the reference's r = 2 h + 1e-9 turned into the threshold on red, and 2 h^2).
 * Bin j is a member of row i when red(i, j) <= thr[i]; a NaN thr: no member.  A member adds
 *   count_j * (uint64) rint(w * 2^s),  w = exp(-(dist / two_h2[i])),
 * to the row's 64-bit sum of its class; dist = red (euclidean) or (2 asin(sqrt(a)))^2 with
 * a = sin(dlat / 2)^2 + (cos lat_j cos lat_i) sin(dlon / 2)^2, d = bin - query (haversine: the reference's
 * utils.distance_pw_haversine order).  s = range_kde_scale_bits: the largest s <= 52 with total count * 2^s < 2^62.
 * A w that is no number in [0, 1] counts as 0 (1 above 1).  With I_c the sums of a row, S their exact sum and m the
 * smallest non-zero one:  prior[c] = ((double) I_c + (double) m) / ((double) S + (double) C * (double) m), and
 * 1.0 / C when S == 0.  Scores, the three integers and their flags: as range_neighbor_rank.  Integer sums: no result
 * depends on the launch geometry, the stream, the order of the bins, or on whether a bin of count n is installed as
 * n bins of count 1, bit for bit. */
#define RANGE_KDE_MAX_CLASSES 16384 /* one uint64 row of a query must fit the CU's LDS */

/* The launch plan: out[0] = queries of a workgroup (G), [1] = query groups, [2] = workgroups over the groups,
 * [3] = chunks of the bins, [4] = LDS bytes, [5] = workspace bytes of the partial sums (0 with one chunk),
 * [6] = scale bits s, [7] = tiles of bins.  RANGE_ERR_INVALID: B or M outside 1 .. 2^31 - 1, C outside
 * 1 .. RANGE_KDE_MAX_CLASSES, total_count outside M .. 2^31 - 1, a negative argument. */
int range_kde_plan(int64_t B, int64_t M, int32_t C, int64_t total_count, int64_t max_grid, int32_t chunks,
                   int64_t* out8_host);

/* Installs M bins: lonlat_host (M, 2), classes_host (M) in [0, C), counts_host (M) int32 >= 1.  Host arrays,
 * synchronous, replaces an earlier set of either kind.  RANGE_ERR_INVALID: a count < 1, a class outside [0, C)
 * (names the first), counts that sum beyond 2^31 - 1, C beyond RANGE_KDE_MAX_CLASSES.  On such a set
 * range_neighbor_select works unchanged (the kde_nb-th bin) and RANGE_NEIGHBOR_CELL calls are refused; the
 * range_kde_* calls below are refused (RANGE_ERR_STATE) on a set installed by range_set_neighbors. */
int range_set_kde_points(range_ctx* ctx, const double* lonlat_host, const int32_t* classes_host,
                         const int32_t* counts_host, int64_t M, int32_t C, int32_t haversine);
int32_t range_kde_scale_bits(const range_ctx* ctx); /* 0: no weighted set installed */

/* The three rank integers of B queries: q_dev (B, 2), thr_dev (B), two_h2_dev (B) float64; img_dev, img_kind,
 * labels_dev and the outputs as range_neighbor_rank. */
int range_kde_rank(range_ctx* ctx, const double* q_dev, const double* thr_dev, const double* two_h2_dev, int64_t B,
                   const void* img_dev, int32_t img_kind, const int32_t* labels_dev, int32_t* greater_dev,
                   int32_t* tied_after_dev, int32_t* argmax_dev, range_stream_t stream);
int range_kde_rank_grid(range_ctx* ctx, const double* q_dev, const double* thr_dev, const double* two_h2_dev, int64_t B,
                        const void* img_dev, int32_t img_kind, const int32_t* labels_dev, int32_t* greater_dev,
                        int32_t* tied_after_dev, int32_t* argmax_dev, int64_t max_grid, int32_t chunks,
                        range_stream_t stream);

/* The (B, C) float64 priors; the _grid form also gives the (B, C) uint64 sums (sums_dev, or NULL) and may leave
 * prior_dev NULL. */
int range_kde_prior(range_ctx* ctx, const double* q_dev, const double* thr_dev, const double* two_h2_dev, int64_t B,
                    double* prior_dev, range_stream_t stream);
int range_kde_prior_grid(range_ctx* ctx, const double* q_dev, const double* thr_dev, const double* two_h2_dev, int64_t B,
                         double* prior_dev, uint64_t* sums_dev, int64_t max_grid, int32_t chunks,
                         range_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
