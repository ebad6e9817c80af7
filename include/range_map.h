/* range_map.h - C ABI of the embedding map in librange_hip.so (MI355X / gfx950).
 *
 * Replaces the arithmetic of the reference's range/evaluation/visualize_embeddings.py:120-139: the
 * column standardisation (:121-125), FastICA(n_components=3, random_state=2001,
 * whiten='unit-variance', max_iter=1000) fit and transform (:132-135) and the per-component
 * skimage.exposure.equalize_hist (:138-139).  The c x c and d x d host algebra (eigen-decompositions,
 * the symmetric decorrelation, the convergence limit) stays on the host (range_amd/embedding_map.py);
 * everything that touches the n rows runs behind these entry points and the probe's
 * (range_probe_colstats / _scale_rows / _gemm), in float64.
 *
 * Conventions: as range_probe.h.  The entry points take a range_probe_ctx; c is the number of
 * components, 1 <= c <= RANGE_MAP_MAX_C.  max_grid = 0 lets the launch plan choose the grid, g > 0
 * caps it at g workgroups (the results do not depend on it, bit for bit).
 */
#ifndef RANGE_MAP_H
#define RANGE_MAP_H

#include "range_probe.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RANGE_MAP_MAX_C 8
#define RANGE_MAP_MAX_BINS 1024

/* The launch plan of n rows and c components (a pure function of its arguments, no device):
 * out[0] = rows of one ICA-step slab, [1] = slabs, [2] = workgroups of the ICA step, [3] = workspace
 * bytes, [4] = rows of one projection trip of a workgroup, [5] = workgroups of the projection,
 * [6] = rows of one equalisation trip of a workgroup, [7] = workgroups of the equalisation. */
int range_map_plan(int64_t n, int32_t c, int64_t max_grid, int64_t* out8_host);

/* Sizes the context's workspace for range_map_ica_step on n rows and c components.  This is the
 * only call of this header that may allocate; range_map_ica_step refuses a shape whose slabs do not fit
 * the workspace reserved so far (a smaller shape than the reserved one runs). */
int range_map_reserve(range_probe_ctx* ctx, int64_t n, int32_t c);

/* Y[k*ldy + i] = sum_j K[k*d + j] * (X[i*ldx + j] - mean[j]); X (n x d, ldx) is read once.
 * mean may be null (X is centred already).  K (c x d, dense) and mean live on the device. */
int range_map_project(range_probe_ctx* ctx, const double* X_dev, int64_t n, int32_t d, int64_t ldx,
                      const double* mean_dev, const double* K_dev, int32_t c, double* Y_dev,
                      int64_t ldy, int64_t max_grid, range_stream_t stream);

/* The data part of one parallel-FastICA step (sklearn _ica_par with the logcosh contrast):
 *   out[k*c + l] = sum_i tanh(w_k . y_i) * Y[l*ldy + i],   out[c*c + k] = sum_i (1 - tanh^2(w_k . y_i))
 * with W (c x c, row-major) read from the host at the call.  The sums are formed in one fixed order
 * that depends on n and c alone: same bits on every run, stream and grid. */
int range_map_ica_step(range_probe_ctx* ctx, const double* Y_dev, int64_t n, int64_t ldy, int32_t c,
                       const double* W_host, double* out_dev, int64_t max_grid,
                       range_stream_t stream);

/* S[i*c + k] = sum_l M[k*c + l] * Y[l*ldy + i]  (n x c, dense); M (c x c) read from the host. */
int range_map_sources(range_probe_ctx* ctx, const double* Y_dev, int64_t n, int64_t ldy, int32_t c,
                      const double* M_host, double* S_dev, int64_t max_grid, range_stream_t stream);

/* Histogram equalisation of one column x[i*ldx], i < n (skimage.exposure.equalize_hist of a float
 * image): counts = numpy.histogram(x, nbins)[0] with edges (nbins + 1, numpy.linspace(first, last),
 * on the device) - the index from (x - first) / (last - first) * nbins, corrected against the edges,
 * the last bin closed - then out[i*ldo] = numpy.interp(x, bin centres, cumsum(counts) / n).
 * counts (nbins, uint64, device) is an output.  Values outside [first, last] are not counted; when none
 * is inside, every output is NaN.  The edges must increase strictly: a range of a few ulps, where
 * numpy.linspace repeats edges, is not covered. */
int range_map_equalize(range_probe_ctx* ctx, const double* x_dev, int64_t n, int64_t ldx,
                       const double* edges_dev, int32_t nbins, uint64_t* counts_dev, double* out_dev,
                       int64_t ldo, int64_t max_grid, range_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
