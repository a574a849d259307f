/*
 * g2048_tlearn.h -- the C-ABI of libg2048_tlearn_hip.so: the transformer policy's PPO loss and gradient pass (the network of
 * g2048_tpolicy_pack / g2048_tpolicy_forward in g2048.h, models/transformer.py:4-40 of the reference). A third, small library next
 * to libg2048_hip.so (include/g2048.h) and libg2048_train_hip.so (include/g2048_train.h), built from csrc/g2048_tpolicy_grad.hip;
 * it has its own error string and version, and needs nothing of the other two at run time. The conventions are g2048.h's: device
 * pointers, `stream` a hipStream_t (NULL: the default stream), G2048_OK or an error code with a message in
 * g2048_tlearn_last_error() (per thread), argument checks before any device call, n == 0 returns G2048_OK and does nothing.
 *
 * The function that is differentiated is PPOAgent.update()'s loss (agents/ppo_agent.py:378-400) on the module's two heads, the
 * module in eval mode (dropout off):
 *     probs, value = model(codes / 15)
 *     logp   = log(probs[i, actions[i]])                      Categorical(probs=probs).log_prob, probabilities clamped at f32 eps
 *     ratio  = exp(logp - old_log_probs)
 *     actor  = -mean(min(ratio adv, clamp(ratio, 1 - clip, 1 + clip) adv))
 *     vloss  = mean((value[:, 0] - returns)^2)
 *     ent    = mean(Categorical(probs=probs).entropy())
 *     loss   = actor + value_coef vloss - entropy_coef ent
 * One shared trunk, one parameter set, one gradient. f32 only: the pass reads the PLAIN f32 parameter buffer (g2048_tpolicy_pack's
 * input), whatever precision the acting blob was packed in.
 */
#ifndef G2048_TLEARN_H
#define G2048_TLEARN_H
#include "g2048.h"
#ifdef __cplusplus
extern "C" {
#endif

#define G2048_TLEARN_ABI_VERSION 1
#define G2048_TLEARN_BATCH_MAX 1024      /* boards per call: 16,384 tokens */

G2048_API const char *g2048_tlearn_last_error(void);
G2048_API int g2048_tlearn_abi_version(void);

/* Bytes of the workspace g2048_tpolicy_loss_grad needs for n boards; 0 for a refused shape: n == 0, n > G2048_TLEARN_BATCH_MAX,
 * dim_ff not a multiple of 32 in 32 .. 65536, n_layers outside 1 .. 64. */
G2048_API size_t g2048_tpolicy_grad_workspace(size_t n, int dim_ff, int n_layers);

/* boards: uint8 [n][16] codes; plain_f32: the plain parameter buffer; actions int64 [n] (the kernel reads actions & 3);
 * old_log_probs, advantages, returns float [n]. Outputs: grad_out, d loss / d parameter for every float of plain_f32 in its
 * layout (the two LayerNorm-eps slots per layer 0), overwritten, never accumulated into; losses4_out = {loss, actor, value loss,
 * entropy}; probs_out float [n][4]; value_out float [n]. A sequence of launches on `stream` over the workspace, no atomics, every
 * output element one fixed-order accumulation: two calls give the same bits, and a board's place in the batch changes only the
 * order of the sums over the batch. Nothing past row n or past workspace_bytes is read or written. Alignment: boards, plain_f32,
 * grad_out, probs_out, workspace 16 bytes; actions 8; the rest 4. clip_epsilon, value_coef, entropy_coef: finite, not negative. */
G2048_API int g2048_tpolicy_loss_grad(const void *boards, const float *plain_f32, const int64_t *actions, const float *old_log_probs,
                                      const float *advantages, const float *returns, size_t n, int dim_ff, int n_layers,
                                      float clip_epsilon, float value_coef, float entropy_coef, float *grad_out, float *losses4_out,
                                      float *probs_out, float *value_out, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
