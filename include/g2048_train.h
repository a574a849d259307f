/*
 * g2048_train.h -- the C-ABI of libg2048_train_hip.so: the hybrid agent's Q-network in TRAINING mode, with the reference's live
 * dropout (agents/hybrid.py:1038-1044: DQNAgent.train_step never calls .eval(), so all three forwards of a train step run
 * nn.TransformerEncoderLayer's four dropout sites). A second, small library next to libg2048_hip.so (include/g2048.h), built from
 * csrc/g2048_qnet_train.hip; it has its own error string and version, and needs nothing of the main library at run time. The
 * conventions are g2048.h's: device pointers, `stream` a hipStream_t (NULL: the default stream), G2048_OK or an error code with
 * a message in g2048_train_last_error() (per thread), argument checks before any device call, n == 0 returns G2048_OK and does
 * nothing. Acting (g2048_qnet_forward, g2048_qnet_select_actions, the play kernels) has no dropout here or there.
 *
 * Dropout (DESIGN.md "RNG", domain 12). Per library call with index c: (k0, k1) = rng_keys(seed, 12, c). Element e of site s of
 * encoder layer L is kept iff rng_draw(k0, k1, ((4 L + s) << 32) | e, 0) >= floor(p[s] 2^32); a kept element is multiplied by
 * float32(1 / (1 - p[s])), a dropped one by 0 -- a product in both directions, so a dropped inf or NaN becomes NaN as in torch. The
 * sites, in the order torch's training-mode layer draws:
 *   s = 0  the attention probabilities, masked before P.V (the row's max and sum are of the unmasked scores);
 *          e = (head n + query) n + key, the site's matrix is [8 n][n]
 *   s = 1  dropout1 on out_proj's output, before the residual add; e = row 128 + feature, [n][128]
 *   s = 2  dropout on the ReLU'd hidden layer; e = row dim_ff + feature, [n][dim_ff]
 *   s = 3  dropout2 on linear2's output, before the residual add; e = row 128 + feature, [n][128]
 * p: four doubles on the host, each finite with 0 <= p < 1, shared by all layers. A site with p[s] == 0 is not hashed; with all
 * four 0 the two passes launch the kernels of g2048_qnet_forward_batch / g2048_qnet_loss_grad and give their bits. No mask is
 * stored: the backward regenerates every one.
 */
#ifndef G2048_TRAIN_H
#define G2048_TRAIN_H
#include "g2048.h"
#ifdef __cplusplus
extern "C" {
#endif

#define G2048_TRAIN_ABI_VERSION 1

G2048_API const char *g2048_train_last_error(void);
G2048_API int g2048_train_abi_version(void);

/* g2048_qnet_forward_batch (g2048.h) with the masks of call `call_index`. workspace: g2048_qnet_batch_workspace(n, dim_ff) bytes;
 * the forward stores nothing more. */
G2048_API int g2048_qnet_forward_batch_dropout(const void *boards, const float *plain_f32, float *q_out, size_t n, int dim_ff, int n_layers,
                                               const double *p4, uint64_t seed, uint64_t call_index, void *workspace, void *stream);

/* Bytes of the workspace g2048_qnet_loss_grad_dropout needs (g2048_qnet_grad_workspace's plus one [n][128] array: the gradient
 * at a dropped projection's output); 0 for n == 0, n > G2048_QNET_BATCH_MAX or a bad shape. */
G2048_API size_t g2048_qnet_train_workspace(size_t n, int dim_ff, int n_layers);

/* g2048_qnet_loss_grad (g2048.h) with the masks of call `call_index`: the forward keeps the DROPPED attention output and the
 * DROPPED hidden layer, the backward regenerates the masks. Same outputs, same rules (no atomics, fixed order, two calls give the
 * same bits, nothing past row n is written). workspace: g2048_qnet_train_workspace(n, dim_ff, n_layers) bytes. */
G2048_API int g2048_qnet_loss_grad_dropout(const void *boards, const float *plain_f32, const int64_t *actions, const float *targets,
                                           const float *weights, size_t n, int dim_ff, int n_layers, const double *p4, uint64_t seed,
                                           uint64_t call_index, float *grad_out, float *td_out, float *loss_out, float *q_out,
                                           void *workspace, void *stream);

/* The keep bits (uint8, 1 = kept) of rows [first_row, first_row + rows) of site `site`'s matrix of layer `layer` for n boards,
 * written by the function the kernels draw with: keep_out[(row - first_row) columns + column]. p: that site's probability. */
G2048_API int g2048_qnet_dropout_mask(uint64_t seed, uint64_t call_index, int layer, int site, double p, size_t n, int dim_ff,
                                      size_t first_row, size_t rows, uint8_t *keep_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
