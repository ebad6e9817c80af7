/* librange_hip.so - training a CSP location encoder and its class head on the GPU.
 *
 * The reference's supervised stage (location_models/csp/main/trainer.py:753-797 -> trainer_helper.py:113-174:
 * losses.py:395-470 embedding_loss without 'user', under torch.optim.Adam) on the whole LocationImageEncoder: the
 * feed-forward net behind the 'gridcell' / 'theory' features (module.py:104-229) and class_emb W_c (C, num_filts).
 * A step has B batch locations with labels and Bg background locations, R = B + Bg rows:
 *
 *   features  float64 sines and cosines rounded once to float32 - the rows range_csp_encode forms; no gradient
 *   layer l   Z = X W^T + b, A = act(Z), D = dropout(A), S = D + X where the layer's skip is live (a hidden layer
 *             whose input and output widths agree, skip set), Y = LayerNorm(S) for the hidden layers with use_layn
 *             (biased variance, eps 1e-5 under the root, affine); the last layer has activation and dropout only
 *   head      p = sigmoid(E W_c^T), the loss of include/range_headfit.h on the embeddings E
 *   backward  dE = G W_c; per layer from the last: LayerNorm backward (dgamma = sum_r dY xhat, dbeta = sum_r dY, dS
 *             by the three-term formula), dX += dS where the skip is live, dZ = dS * mask * act'(Z), db = sum_r dZ,
 *             dW = dZ^T X, dX += dZ W
 *   Adam      torch.optim.Adam's (L2 weight decay into the gradient, bias corrections by the step count, no amsgrad)
 *             on every W_l, b_l, gamma_l, beta_l and W_c with one lr / weight_decay
 *
 * float32 throughout, exact float32 products: every logit and every Z entry one k-ordered chain from 0; dW, db,
 * dgamma, dbeta one chain ordered by row index; dE one chain ordered by class index whatever the panel width; dX = dZ W
 * one chain ordered by output column (the skip's dS added behind it); LayerNorm's row sums in the encoder's fixed
 * order; no atomics.  No result depends on the grid, the stream or the class-panel width.  The embeddings of a fit are
 * the bits range_csp_encode returns for the same network.
 *
 * Dropout (dropout_p in [0, 1); 0: none): in every layer, the last included.  Entry (row r of the step, column c) of
 * layer l at step count t is kept when (mix(mix(key ^ r) ^ c) >> 8) < floor((1 - p) 2^24), key = mix(mix(mix(mix(seed
 * low 32 bits) ^ seed high 32 bits) ^ (uint32) t) ^ l), mix(x): x ^= x >> 16, x *= 0x7feb352d, x ^= x >> 15, x *=
 * 0x846ca68b, x ^= x >> 16 on 32 bits; kept entries are scaled by 1 / (1 - p).  t is the fit's step count when the
 * call starts, for range_cspfit_grad and range_cspfit_loss as for the step they precede.
 *
 * A context holds at most one fit (range_cspfit_begin): the parameters, Adam's two moments, the step count.  It is
 * independent of the installed inference network (range_set_csp / range_set_csp_head) and of a class-head fit
 * (range_headfit_begin); neither disturbs the other.  Every call that takes a stream is asynchronous on it; a call
 * whose workspace has to grow synchronises the device once.  The fit has ONE workspace: calls of one context on two
 * streams must be ordered by the caller (an event, or a synchronisation), as two steps of one fit have to be anyway.
 *
 * Rows of a call: `lonlat` (N, 2) float64 (lon, lat) degrees on the device, `rows` B int32 ids into it (NULL: rows
 * 0 .. B - 1, which needs N >= B; an id outside 0 .. N - 1 is clamped), `labels` B int32 (a label outside 0 .. C - 1
 * matches no column), `bg_lonlat` (Bg, 2) float64 (NULL with Bg = 0).  A NaN or infinite coordinate makes its row's
 * embedding NaN and with it every gradient the row reaches, as in torch.
 * Envelope: the encoder's (range_set_csp) and the head fit's: F <= 64, widths <= 1024, <= 8 hidden layers, 1 <= C <=
 * 32768, 1 <= B, 0 <= Bg, B + Bg <= 8192, and a workspace of at most 512 MiB (range_cspfit_plan).
 *
 * UNPACKED ORDER of range_cspfit_grad and range_cspfit_params, float32: per layer l = 0 .. n_layers - 1 its W (out, in)
 * row-major, b (out), and - only for a hidden layer with use_layn - gamma (out), beta (out); then class_emb (C,
 * num_filts) row-major.  range_cspfit_param_count() floats in all.
 *
 * `loss3`: as in include/range_headfit.h.  Return codes and range_last_error(): include/range_hip.h.
 */
#ifndef RANGE_CSPFIT_H
#define RANGE_CSPFIT_H

#include "range_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The launch plan of a step on `rows` = B + Bg rows (host_plan.h: cspfit_plan; needs no GPU), out16: [0] panel_cols,
 * [1] n_panels, [2] the head's tile_rows, [3] LayerNorm lanes per row, [4] the features launch's grid, [5] the row
 * launches' grid, [6] the grid of dE = G W_c, [7] the head's gradient grid of panel 0, [8] its update grid of panel
 * 0, [9] lds_bytes (the largest launch), [10] ws_bytes (<= 512 MiB), [11] the unpacked parameter count, [12] the
 * stored (packed) floats per copy, [13] the widest layer side, [14] - [15] 0.  kind .. use_layn: as range_set_csp. */
int range_cspfit_plan(int32_t kind, int32_t F, int32_t n_layers, const int32_t* widths, int32_t skip, int32_t use_layn,
                      int32_t C, int64_t rows, int64_t max_grid, int32_t panel_cols, int64_t* out16);

/* Starts a fit, replacing an earlier one: the network as range_set_csp takes it (all pointers on the HOST), class_emb
 * (C, num_filts) row-major float32 on the host or NULL for zeros; Adam's moments zero; the step count 0.
 * Synchronises the device. */
int range_cspfit_begin(range_ctx* ctx, int32_t kind, const double* freq_host, int32_t F, int32_t n_layers,
                       const int32_t* widths, const float* const* weights, const float* const* biases,
                       const float* const* ln_gamma, const float* const* ln_beta, int32_t act, int32_t skip,
                       int32_t use_layn, const float* class_emb, int32_t C);
int32_t range_cspfit_classes(const range_ctx* ctx);       /* 0: no fit begun */
int32_t range_cspfit_width(const range_ctx* ctx);         /* num_filts */
int64_t range_cspfit_steps(const range_ctx* ctx);
int64_t range_cspfit_param_count(const range_ctx* ctx);   /* floats of the unpacked order */

/* One Adam step; every parameter and moment is updated in place, the step count goes up by one. */
int range_cspfit_step(range_ctx* ctx, const double* lonlat_dev, int64_t N, const int32_t* rows, const int32_t* labels,
                      int32_t B, const double* bg_lonlat_dev, int32_t Bg, double rand_sample_weight, double lr, double beta1,
                      double beta2, double eps, double weight_decay, double dropout_p, uint64_t dropout_seed, float* loss3,
                      range_stream_t stream);
/* max_grid: a smaller cap on every launch's grid (0: none); panel_cols: a narrower class panel (0: the plan's) - for
 * tests: neither changes a bit of any result. */
int range_cspfit_step_grid(range_ctx* ctx, const double* lonlat_dev, int64_t N, const int32_t* rows, const int32_t* labels,
                           int32_t B, const double* bg_lonlat_dev, int32_t Bg, double rand_sample_weight, double lr,
                           double beta1, double beta2, double eps, double weight_decay, double dropout_p,
                           uint64_t dropout_seed, float* loss3, int64_t max_grid, int32_t panel_cols, range_stream_t stream);

/* Every gradient at the current parameters into `grads` (range_cspfit_param_count() float32 on the device, the
 * unpacked order) - the bits a step would feed to Adam; nothing is updated. */
int range_cspfit_grad(range_ctx* ctx, const double* lonlat_dev, int64_t N, const int32_t* rows, const int32_t* labels,
                      int32_t B, const double* bg_lonlat_dev, int32_t Bg, double rand_sample_weight, double dropout_p,
                      uint64_t dropout_seed, float* grads, float* loss3, range_stream_t stream);
int range_cspfit_grad_grid(range_ctx* ctx, const double* lonlat_dev, int64_t N, const int32_t* rows, const int32_t* labels,
                           int32_t B, const double* bg_lonlat_dev, int32_t Bg, double rand_sample_weight, double dropout_p,
                           uint64_t dropout_seed, float* grads, float* loss3, int64_t max_grid, int32_t panel_cols,
                           range_stream_t stream);

/* The loss alone, the forward pass under the same dropout.  `emb` (NULL: not wanted): the (B + Bg, num_filts) float32
 * embeddings of the call's rows on the device. */
int range_cspfit_loss(range_ctx* ctx, const double* lonlat_dev, int64_t N, const int32_t* rows, const int32_t* labels,
                      int32_t B, const double* bg_lonlat_dev, int32_t Bg, double rand_sample_weight, double dropout_p,
                      uint64_t dropout_seed, float* loss3, float* emb, range_stream_t stream);

/* Every current parameter in the unpacked order, float32 on the device. */
int range_cspfit_params(range_ctx* ctx, float* params, range_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* RANGE_CSPFIT_H */
