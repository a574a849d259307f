/*
 * g2048_ttrain.h -- the C-ABI of libg2048_ttrain_hip.so: the transformer policy's PPO loss and gradient pass and its forward in
 * TRAINING mode, with the encoder's live dropout. models/transformer.py builds nn.TransformerEncoderLayer with torch's default
 * dropout = 0.1 and PPOAgent.update() (agents/ppo_agent.py:357-416) never puts a network into eval mode, so both critic forwards
 * of its advantage block and the forward of every epoch run the layer's four dropout sites. A fifth, small library next to
 * libg2048_tlearn_hip.so (include/g2048_tlearn.h, the eval-mode pass, whose export table is closed), built from
 * csrc/g2048_tpolicy_train.hip; it has its own error string and version, and needs nothing of the others at run time. The
 * conventions are g2048.h's: device pointers, `stream` a hipStream_t (NULL: the default stream), G2048_OK or an error code with a
 * message in g2048_ttrain_last_error() (per thread), argument checks before any device call, n == 0 returns G2048_OK and does
 * nothing. Acting (g2048_tpolicy_forward, the play kernels) has no dropout here or there.
 *
 * Dropout (DESIGN.md "RNG", domain 13). Per library call with index c: (k0, k1) = rng_keys(seed, 13, c). Element e of site s of
 * encoder layer L is kept iff rng_draw(k0, k1, ((4 L + s) << 32) | e, 0) >= floor(p[s] 2^32); a kept element is multiplied by
 * float32(1 / (1 - p[s])), a dropped one by 0 -- a product, not a select, so a NaN in a dropped position stays a NaN as in torch.
 * The sites, in the order torch's training-mode layer draws them, for n boards of 16 tokens (token = 16 board + cell):
 *   s = 0  the attention probabilities, after the softmax (its max and sum are of the unmasked scores), before P.V;
 *          the site's matrix is [64 n][16], e = ((board 4 + head) 16 + query) 16 + key
 *   s = 1  dropout1 on out_proj's output, before the residual add; [16 n][64], e = token 64 + feature
 *   s = 2  dropout on relu(linear1 ..); [16 n][dim_ff], e = token dim_ff + feature
 *   s = 3  dropout2 on linear2's output, before the residual add; as s = 1
 * p4: four doubles on the host, each in [0, 1) (a NaN is refused), shared by all layers. A site with p[s] == 0 is not hashed; with
 * all four 0 the passes launch the kernels of g2048_tpolicy_loss_grad in its order and give its bits. No mask is stored: the
 * backward regenerates every one, and recomputes the hidden layer with the mask the forward used.
 */
#ifndef G2048_TTRAIN_H
#define G2048_TTRAIN_H
#include "g2048.h"
#ifdef __cplusplus
extern "C" {
#endif

#define G2048_TTRAIN_ABI_VERSION 1

G2048_API const char *g2048_ttrain_last_error(void);
G2048_API int g2048_ttrain_abi_version(void);

/* Bytes of the workspace the two passes below need for n boards: g2048_tpolicy_grad_workspace(n, dim_ff, n_layers)
 * (g2048_tlearn.h) plus ONE [16 n][64] float array, the gradient leaving a LayerNorm backward times the multipliers of site 1 or
 * 3 (what enters the dropped projection's weight and data gradients); a multiple of 16. 0 for the shapes that query refuses:
 * n == 0, n > 1024 (G2048_TLEARN_BATCH_MAX), dim_ff not a multiple of 32 in 32 .. 65536, n_layers outside 1 .. 64. */
G2048_API size_t g2048_tpolicy_train_workspace(size_t n, int dim_ff, int n_layers);

/* g2048_tpolicy_loss_grad (g2048_tlearn.h) with the masks of call `call_index`: the same arguments, outputs, alignments and rules
 * (no atomics, every output element one fixed-order accumulation, two calls with the same (seed, call_index) give the same bits,
 * nothing past row n or past workspace_bytes is read or written, no workspace element is read before the call wrote it, the
 * LayerNorm-eps slots of grad_out are 0). The masks belong to positions in the batch, not to boards. workspace:
 * g2048_tpolicy_train_workspace(n, dim_ff, n_layers) bytes. */
G2048_API int g2048_tpolicy_loss_grad_dropout(const void *boards, const float *plain_f32, const int64_t *actions, const float *old_log_probs,
                                              const float *advantages, const float *returns, size_t n, int dim_ff, int n_layers,
                                              const double *p4, uint64_t seed, uint64_t call_index, float clip_epsilon, float value_coef,
                                              float entropy_coef, float *grad_out, float *losses4_out, float *probs_out, float *value_out,
                                              void *workspace, size_t workspace_bytes, void *stream);

/* The training-mode forward alone, in f32 from the plain buffer: the forward launches of the pass above and the two heads.
 * probs_out float [n][4], value_out float [n]; at equal (seed, call_index) they are, bit for bit, what
 * g2048_tpolicy_loss_grad_dropout writes there. Alignment: boards, plain_f32, probs_out, workspace 16 bytes; value_out 4.
 * workspace: g2048_tpolicy_train_workspace(n, dim_ff, n_layers) bytes. */
G2048_API int g2048_tpolicy_forward_dropout(const void *boards, const float *plain_f32, size_t n, int dim_ff, int n_layers, const double *p4,
                                            uint64_t seed, uint64_t call_index, float *probs_out, float *value_out, void *workspace,
                                            size_t workspace_bytes, void *stream);

/* The keep bits (uint8, 1 = kept) of rows [first_row, first_row + rows) of site `site`'s matrix of layer `layer` (0 .. 63) for n
 * boards (at most 1024), written by the function the kernels draw with: keep_out[(row - first_row) columns + column]. p: that
 * site's probability. */
G2048_API int g2048_tpolicy_dropout_mask(uint64_t seed, uint64_t call_index, int layer, int site, double p, size_t n, int dim_ff,
                                         size_t first_row, size_t rows, uint8_t *keep_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
