/*
 * g2048_tbf16.h -- the C-ABI of libg2048_tbf16_hip.so: the transformer policy's PPO loss and gradient pass with its FEED-FORWARD
 * products in bf16 on the matrix cores (v_mfma_f32_16x16x32_bf16, f32 accumulation). A ninth, small library next to
 * libg2048_ttrain_hip.so (include/g2048_ttrain.h, whose export table is closed), built from csrc/g2048_tpolicy_bf16.hip; it has its
 * own error string and version, and needs nothing of the others at run time. The conventions are g2048.h's: device pointers,
 * `stream` a hipStream_t (NULL: the default stream), G2048_OK or an error code with a message in g2048_tbf16_last_error() (per
 * thread), argument checks before any device call, n == 0 returns G2048_OK and does nothing.
 *
 * The pass is g2048_tpolicy_loss_grad_dropout's (g2048_ttrain.h; the loss: g2048_tlearn.h) but for the seven products of every
 * encoder layer that have dim_ff as an extent: linear1 forward and its recomputation in the backward, linear2 forward, dW2, dX
 * through linear2, dW1 and dX through linear1. This is NOT a rounding-level change: on the test cases the gradients move by 0.5 ..
 * 15 % of their largest element against the f32 pass (docs/LOG.md R37). The master weights, the gradients, the embedding, the
 * attention, the LayerNorms, the heads, the loss and everything else stay f32.
 *
 * The function. rnd(v): v as float32, rounded to nearest even to bf16.
 *   - Every operand of the seven products is rnd of its value where the f32 pass reads it: x1, W1, h (after the ReLU and the site-2
 *     multiplier), W2, linear2's dY (ds, or ds x the site-3 multipliers) and dh (after the ReLU mask and the site-2 multiplier).
 *   - h and dh are STORED as rnd of those values, bf16 [16 n][dim_ff]; the ReLU mask of dh is h > 0 on the stored value.
 *   - Biases and residuals are added in f32 to the f32 product. A bias gradient is the sum of dY as stored: f32 for linear2's, the
 *     bf16 dh for linear1's.
 *   - Accumulation is f32 in a fixed order, no atomics: two calls give the same bits. Weight gradients keep the split into chunks
 *     of 512 rows and the fixed-order combine; the chunk edges are a function of n alone.
 *   - Dropout: the four sites, the masks (domain 13, the same element indices; g2048_tpolicy_dropout_mask describes them) and the
 *     rule that a site with p == 0 is not hashed are g2048_ttrain.h's. The backward's recomputation of h is bit for bit the forward's.
 */
#ifndef G2048_TBF16_H
#define G2048_TBF16_H
#include "g2048.h"
#ifdef __cplusplus
extern "C" {
#endif

#define G2048_TBF16_ABI_VERSION 1

G2048_API const char *g2048_tbf16_last_error(void);
G2048_API int g2048_tbf16_abi_version(void);

/* Bytes of the workspace g2048_tpolicy_loss_grad_bf16 needs for n boards, T = 16 n tokens:
 *     g2048_tpolicy_train_workspace(n, dim_ff, n_layers) - 2 * (4 - 2) * T * dim_ff + n_layers * 4 * 64 * dim_ff * 2
 * the training pass's workspace with h and dh at 2 bytes an element, plus every layer's packed bf16 weights (W1, W2 and the
 * transpose of each; packed once a call). Smaller than g2048_tpolicy_grad_workspace where 64 n dim_ff exceeds
 * 512 n_layers dim_ff + 4096 n. 0 for the shapes
 * that query refuses: n == 0, n > 1024, dim_ff not a multiple of 32 in 32 .. 65536, n_layers outside 1 .. 64. */
G2048_API size_t g2048_tpolicy_bf16_workspace(size_t n, int dim_ff, int n_layers);

/* g2048_tpolicy_loss_grad_dropout's arguments, outputs, alignments, checks and rules, with the function above. p4: four doubles
 * on the host as there, or NULL: eval mode, the bits of p4 = {0, 0, 0, 0}. workspace: g2048_tpolicy_bf16_workspace bytes. */
G2048_API int g2048_tpolicy_loss_grad_bf16(const void *boards, const float *plain_f32, const int64_t *actions, const float *old_log_probs,
                                           const float *advantages, const float *returns, size_t n, int dim_ff, int n_layers,
                                           const double *p4, uint64_t seed, uint64_t call_index, float clip_epsilon, float value_coef,
                                           float entropy_coef, float *grad_out, float *losses4_out, float *probs_out, float *value_out,
                                           void *workspace, size_t workspace_bytes, void *stream);

/* ---- testing: the three products on their own, so that a test can feed both sides identical rounded bits -------------------
 * Not part of the boundary; the kernels are the pass's. Every array is row-major and 16-byte aligned; an *_bf16 flag says that
 * the array holds bf16 (2 bytes an element) instead of float. 1 <= n <= 16,384 rows. Weights are f32 and are rounded by the
 * pass's pack launch into `workspace`. n == 0 returns G2048_OK. */

/* Y [n][M] = act(rnd(X [n][K]) . rnd(W [M][K])^T + bias [M] (+ res [n][M])), act the ReLU where relu != 0; bias and res may be
 * NULL. K a multiple of 32, M of 16. Kinds (x_bf16, y_bf16): (0, 0), (0, 1), (1, 0). workspace: 2 M K bytes. */
G2048_API int g2048_tbf16_test_linear(const void *x, int x_bf16, const float *w, const float *bias, const float *res, void *y, int y_bf16,
                                      int relu, size_t n, int K, int M, void *workspace, size_t workspace_bytes, void *stream);

/* dX [n][K] = (res [n][K] +) rnd(dY [n][M]) . rnd(W [M][K]), then 0 where mask_bf16 [n][K] (bf16) <= 0; res and mask_bf16 may be
 * NULL. M a multiple of 32, K of 16. Kinds (dy_bf16, dx_bf16): (0, 0), (0, 1), (1, 0). workspace: 2 M K bytes. */
G2048_API int g2048_tbf16_test_dx(const void *dy, int dy_bf16, const float *w, const float *res, const void *mask_bf16, void *dx, int dx_bf16,
                                  size_t n, int M, int K, void *workspace, size_t workspace_bytes, void *stream);

/* dW [M][K] = rnd(dY [n][M])^T . rnd(X [n][K]) and db [M] = the column sums of dY as stored, over chunks of 512 rows combined in
 * order. M and K multiples of 16. Kinds (dy_bf16, x_bf16): (0, 0), (0, 1), (1, 0). workspace: ceil(n / 512) (M K + M) floats. */
G2048_API int g2048_tbf16_test_dw(const void *dy, int dy_bf16, const void *x, int x_bf16, float *dw, float *db, size_t n, int M, int K,
                                  void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
