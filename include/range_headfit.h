/* librange_hip.so - fitting the CSP class head on the GPU from frozen embeddings.
 *
 * The reference's supervised stage (location_models/csp/main/trainer.py:753-797 -> trainer_helper.py:113-174:
 * losses.py:395-470 embedding_loss without 'user', under torch.optim.Adam) with the location encoder frozen is a
 * fit of the one matrix class_emb W (C, F).  For (B, F) embeddings X of a batch with labels y, (Bg, F) embeddings
 * Xbg of background locations, z = x W^T and p = sigmoid(z):
 *
 *   loss = mean_{B x C}(Lpos) + rand_sample_weight * mean_{Bg x C}(Lbg)
 *   Lbg = -log(1 - p + 1e-5);  Lpos the same, except -C log(p + 1e-5) at the label's column
 *
 * A context holds at most one fit: W, Adam's two moments and the step count (range_headfit_begin).  Every call
 * below that takes a stream is asynchronous on it and orders there like any other work; a call whose workspace has
 * to grow synchronises the device once.  float32 throughout; exact float32 products, every logit one k-ordered
 * chain, every gradient entry one chain ordered by row index, the loss sums in a fixed order: the results do not
 * depend on the grid, the stream or the panel width, and no atomics are used.
 *
 * Rows of a call: `feats` (N, F) float32 on the device, `rows` B int32 row ids into it (NULL: rows 0 .. B - 1, which
 * needs N >= B; an id outside 0 .. N - 1 is clamped), `labels` B int32 (a label outside 0 .. C - 1 matches no
 * column: the row then has negatives only), `bg` (Bg, F) float32 (NULL with Bg = 0: no background term).
 * Envelope: 1 <= C <= 32768, 1 <= F <= 1024, 1 <= B, 0 <= Bg, B + Bg <= 8192.
 *
 * `loss3` (NULL in range_headfit_step / range_headfit_grad: not wanted): three float32 on the device -
 * [0] the loss, [1] its batch part mean_{B x C}(Lpos), [2] the mean over the batch rows of -log(p_label + 1e-5)
 * (trainer_helper.py: test()) - all at the weights the call STARTED from.
 *
 * Return codes and range_last_error(): include/range_hip.h.
 */
#ifndef RANGE_HEADFIT_H
#define RANGE_HEADFIT_H

#include "range_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The launch plan of a step on `rows` = B + Bg rows (host_plan.h: headfit_plan; needs no GPU), out8:
 * [0] panel_cols, [1] n_panels, [2] tile_rows, [3] cols_per_pass, [4] the gradient launch's grid of panel 0,
 * [5] the update launch's grid of panel 0, [6] lds_bytes, [7] ws_bytes (<= 256 MiB).  max_grid / panel_cols: as in
 * the _grid calls. */
int range_headfit_plan(int32_t C, int32_t F, int64_t rows, int64_t max_grid, int32_t panel_cols, int64_t* out8);

/* Starts a fit of a (C, F) head, replacing an earlier one: W = w0_host (C, F) row-major float32 on the HOST, or zeros
 * with NULL; Adam's moments zero; the step count 0.  Synchronises the device. */
int range_headfit_begin(range_ctx* ctx, int32_t C, int32_t F, const float* w0_host);
int32_t range_headfit_classes(const range_ctx* ctx);      /* 0: no fit begun */
int32_t range_headfit_width(const range_ctx* ctx);
int64_t range_headfit_steps(const range_ctx* ctx);

/* One step of torch.optim.Adam (betas, eps, L2 weight_decay added to the gradient, bias corrections by the step
 * count, no amsgrad) on the loss above; W and the moments are updated in place, the step count goes up by one. */
int range_headfit_step(range_ctx* ctx, const float* feats, int64_t N, const int32_t* rows, const int32_t* labels, int32_t B,
                       const float* bg, int32_t Bg, double rand_sample_weight, double lr, double beta1, double beta2,
                       double eps, double weight_decay, float* loss3, range_stream_t stream);
/* max_grid: a smaller cap on every launch's grid (0: none); panel_cols: a narrower class panel than the workspace
 * allows, rounded up to whole 32-class tiles (0: the plan's) - for tests: neither changes a bit of any result. */
int range_headfit_step_grid(range_ctx* ctx, const float* feats, int64_t N, const int32_t* rows, const int32_t* labels,
                            int32_t B, const float* bg, int32_t Bg, double rand_sample_weight, double lr, double beta1,
                            double beta2, double eps, double weight_decay, float* loss3, int64_t max_grid, int32_t panel_cols,
                            range_stream_t stream);

/* The gradient of the loss with respect to W at the current weights, dW (C, F) row-major float32 on the device -
 * the bits a step would feed to Adam; nothing is updated. */
int range_headfit_grad(range_ctx* ctx, const float* feats, int64_t N, const int32_t* rows, const int32_t* labels, int32_t B,
                       const float* bg, int32_t Bg, double rand_sample_weight, float* dW, float* loss3, range_stream_t stream);
int range_headfit_grad_grid(range_ctx* ctx, const float* feats, int64_t N, const int32_t* rows, const int32_t* labels,
                            int32_t B, const float* bg, int32_t Bg, double rand_sample_weight, float* dW, float* loss3,
                            int64_t max_grid, int32_t panel_cols, range_stream_t stream);

/* The loss alone (no gradient workspace is written). */
int range_headfit_loss(range_ctx* ctx, const float* feats, int64_t N, const int32_t* rows, const int32_t* labels, int32_t B,
                       const float* bg, int32_t Bg, double rand_sample_weight, float* loss3, range_stream_t stream);
int range_headfit_loss_grid(range_ctx* ctx, const float* feats, int64_t N, const int32_t* rows, const int32_t* labels,
                            int32_t B, const float* bg, int32_t Bg, double rand_sample_weight, float* loss3, int64_t max_grid,
                            int32_t panel_cols, range_stream_t stream);

/* The current W as (C, F) row-major float32 on the device (what range_set_csp_head takes once copied to the host). */
int range_headfit_weights(range_ctx* ctx, float* W, range_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* RANGE_HEADFIT_H */
