/*
 * g2048_tstep.h -- the C-ABI of libg2048_tstep_hip.so: what follows the transformer policy's gradient pass in an epoch of
 * PPOAgent.update (agents/ppo_agent.py:403-416 of the reference): the NaN check on the loss, clip_grad_norm_ and an Adam step over
 * the network of g2048_tpolicy_pack (g2048.h) and the gradient of g2048_tpolicy_loss_grad (g2048_tlearn.h). A fourth, small library
 * next to libg2048_hip.so, libg2048_train_hip.so and libg2048_tlearn_hip.so, built from csrc/g2048_tpolicy_step.hip; it has its
 * own error string and version, and needs nothing of the other three at run time. The conventions are g2048.h's: device pointers,
 * `stream` a hipStream_t (NULL: the default stream), G2048_OK or an error code with a message in g2048_tstep_last_error() (per
 * thread), argument checks before any device call.
 */
#ifndef G2048_TSTEP_H
#define G2048_TSTEP_H
#include "g2048.h"
#ifdef __cplusplus
extern "C" {
#endif

#define G2048_TSTEP_ABI_VERSION 1

G2048_API const char *g2048_tstep_last_error(void);
G2048_API int g2048_tstep_abi_version(void);

/* Bytes of the workspace g2048_tpolicy_adam_step needs, a multiple of 16: one double per partial sum of the norm (at most 1,024,
 * their number a function of the float count alone) and the record its second launch prepares for its third. 0 for a refused
 * shape: dim_ff not a multiple of 32 in 32 .. 65536, n_layers outside 1 .. 64. */
G2048_API size_t g2048_tpolicy_step_workspace(int dim_ff, int n_layers);

/* plain, grad, exp_avg, exp_avg_sq: float [128 + n_layers (16962 + 129 dim_ff) + 139781] in the PLAIN layout, all updated IN PLACE.
 * loss_or_null: the loss the gradient belongs to (g2048_tpolicy_loss_grad's losses4_out), NULL: no loss gate. counters3 =
 * {applied steps, calls skipped for a NaN loss, calls skipped for a norm that is not finite}. Three launches on `stream`:
 *     norm = sqrt(sum grad[i]^2), summed in f64 in an order that depends on the float count alone, over the WHOLE buffer, the two
 *            LayerNorm-eps slots of every layer included: g2048_tpolicy_loss_grad leaves those gradient slots 0, and a caller who
 *            fills grad another way must do the same;
 *     the gate, decided once on the device: a NaN loss (isnan only: +inf is applied) skips the call and counters3[1] += 1; else a
 *            norm that is not finite skips it and counters3[2] += 1; else counters3[0] += 1, and that value t is Adam's step;
 *     c = min(1, (1 / (norm + 1e-6)) max_norm) (max_norm = +inf: no clipping), g = grad c (grad is left clipped, as
 *            clip_grad_norm_ leaves it), m += (g - m)(1 - beta1), v = v beta2 + (g g)(1 - beta2),
 *            p -= (lr / (1 - beta1^t)) (m / (sqrt(v) / sqrt(1 - beta2^t) + eps)), every operation rounded to f32 on its own; 1 - beta
 *            is formed in f64 from the shortest decimal that rounds to the float given (0.999f -> 0.001).
 * The two LayerNorm-eps slots of every layer (the last two floats of a layer's block; blocks start at float 128) are settings: all
 * four buffers keep their bits there. A skipped call writes nothing to the four buffers; norm_out (one float, the norm before
 * clipping) is written on every call. No atomics, nothing depends on the device: two calls give the same bits. Nothing outside
 * the four buffers, counters3, norm_out and workspace_bytes of the workspace is read or written. Alignment: the four buffers and
 * the workspace 16 bytes, counters3 8, loss_or_null and norm_out 4. lr, beta1, beta2, eps finite and not negative, both betas
 * below 1, max_norm > 0. */
G2048_API int g2048_tpolicy_adam_step(float *plain, float *grad, float *exp_avg, float *exp_avg_sq, int dim_ff, int n_layers,
                                      const float *loss_or_null, int64_t *counters3, float lr, float beta1, float beta2, float eps,
                                      float max_norm, float *norm_out, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
