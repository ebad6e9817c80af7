/* range_cluster.h - C ABI of the cluster map in librange_hip.so (MI355X / gfx950).
 *
 * Replaces the arithmetic of the reference's location_models/csp/main/analysis.py:417-432
 * (spa_enc_embed_clustering): the row mask and zero fill (:417-423), the L2 normalisation of the rows (:425-426)
 * and AgglomerativeClustering(n_clusters, cosine, complete linkage) (:431) - i.e. the scikit-learn / scipy code that
 * line runs: the cosine distance matrix and the complete-linkage tree cut at n_clusters.  Everything that touches
 * the n x d features or the n x n distances runs behind these entry points and range_probe_gemm, in float64; the
 * sort of the n - 1 merges and the union-find of the cut are host arithmetic (range_cluster_cut, no device).
 *
 * Complete linkage is reducible, so all mutually nearest pairs of clusters can merge at once: the tree is built in
 * rounds (a few dozen for embeddings, n - 1 at the most), every round a handful of launches and one stream
 * synchronisation for a 4-byte read of its pair count.  No kernel waits on another workgroup.
 *
 * Conventions: as range_probe.h.  The entry points take a range_probe_ctx.  max_grid = 0 lets the launch plan
 * choose the grids, g > 0 caps them at g workgroups; the results do not depend on it, on the stream or on the
 * call, bit for bit.
 */
#ifndef RANGE_CLUSTER_H
#define RANGE_CLUSTER_H

#include "range_probe.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RANGE_CLUSTER_MAX_ROWS 131072
/* a failure that no input should be able to cause (a linkage round without a reciprocal pair) */
#define RANGE_ERR_INTERNAL (-5)

/* The launch plan of n rows of d features (a pure function of its arguments, no device):
 * out[0] = bytes of the n x n matrix, [1] = workspace bytes, [2] = workgroups of the normaliser, [3] = tiles of
 * the distance finish, [4] = its workgroups, [5] = workgroups of the first row scan, [6] = column chunks of a row
 * in the merges, [7] = rows a thread of the one-workgroup list kernels owns. */
int range_cluster_plan(int64_t n, int32_t d, int64_t max_grid, int64_t* out8_host);

/* Sizes the context's workspaces for range_cluster_distances and range_cluster_linkage on n rows of d features.
 * This is the only call of this header that may allocate; the others refuse a shape that does not fit what is
 * reserved (a smaller shape than the reserved one runs). */
int range_cluster_reserve(range_probe_ctx* ctx, int64_t n, int32_t d);

/* E[i,:] = y / |y|_2 and norm2[i] = |y|^2 (norm2 may be null), X (n x d, ldx) read once.  mask null: y = X[i,:].
 * mask (n, device): y = X[i,:] * mask[i], then sqrt(1/d) is added to every entry of y that equals 0 - in masked
 * and unmasked rows alike (analysis.py:421-423).  E may be X. */
int range_cluster_normalize(range_probe_ctx* ctx, const double* X_dev, int64_t n, int32_t d, int64_t ldx,
                            const double* mask_dev, double* E_dev, int64_t lde, double* norm2_dev,
                            int64_t max_grid, range_stream_t stream);

/* D[i][j] = max(0, 1 - E[i,:] . E[j,:]) for i != j, +inf for i == j; D (n x n, ldd), n >= 2.  The products come
 * from the float64 matrix cores (the lower triangle of E E^T); D[i][j] and D[j][i] are the same bits. */
int range_cluster_distances(range_probe_ctx* ctx, const double* E_dev, int64_t n, int32_t d, int64_t lde,
                            double* D_dev, int64_t ldd, int64_t max_grid, range_stream_t stream);

/* Complete linkage of the symmetric distance matrix D (n x n, ldd; the diagonal is never read), which is destroyed.
 * merges (n - 1, 2, int32) and heights (n - 1) receive the merge record in emission order: round by round, inside
 * a round by ascending first row; pair (i, j), i < j, joins the clusters that then hold rows i and j at the
 * complete-linkage distance heights[t].  Nearest neighbours are taken under the order (distance, then lower
 * index).  *rounds_host (may be null) = the rounds taken, n - 1 at the most.  Synchronises the stream once a round.
 * A round without a reciprocal pair - impossible for a symmetric matrix without NaN - returns RANGE_ERR_INTERNAL. */
int range_cluster_linkage(range_probe_ctx* ctx, double* D_dev, int64_t n, int64_t ldd, int32_t* merges_dev,
                          double* heights_dev, int32_t* rounds_host, int64_t max_grid, range_stream_t stream);

/* Host-clock times of the context's last range_cluster_linkage, in milliseconds: out[0] = until the first round's
 * pair count arrived (the scan of all n rows), out[1] = the remaining rounds.  The loop synchronises once a round
 * anyway; nothing is added to it.  For tools/cluster_map_bench.py. */
int range_cluster_stage_times(range_probe_ctx* ctx, double* out2_host);

/* The cut (host arrays, no device): the merges sorted stably by height; labels (n, int32, may be null) = the
 * clusters after the first n - n_clusters of them, numbered by first occurrence (the cluster of row 0 is 0, the next
 * new cluster met going down the rows is 1, ...); Z (n - 1, 4, may be null) = scipy's linkage matrix of the tree. */
int range_cluster_cut(int64_t n, const int32_t* merges_host, const double* heights_host, int64_t n_clusters,
                      int32_t* labels_host, double* Z_host);

#ifdef __cplusplus
}
#endif
#endif
