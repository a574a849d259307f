/*
 * g2048_tpolicy_collect.h -- the C-ABI of libg2048_tpolicy_collect_hip.so: the transformer policy's experience collection (the
 * acting loop of train.py:55-90 with the reference's TransformerModel, models/transformer.py:4-40, in eval mode: its
 * probabilities sampled under the env's valid-move mask as PPOAgent.get_action samples, agents/ppo_agent.py:211-221, then
 * Game2048Env.step and the auto-reset) in one kernel launch. `steps` moves of `n` environments are played, and every trajectory
 * row g2048.RolloutCollector keeps is written by that launch. A small library next to libg2048_hip.so (include/g2048.h), built
 * from csrc/g2048_tpolicy_collect.hip; it has its own error string and version, and needs nothing of the main library at run
 * time. The conventions are g2048.h's: device pointers, `stream` a hipStream_t (NULL: the default stream), G2048_OK or an error
 * code with a message in g2048_tpolicy_collect_last_error() (per thread), argument checks before any device call, n == 0
 * returns G2048_OK and does nothing.
 */
#ifndef G2048_TPOLICY_COLLECT_H
#define G2048_TPOLICY_COLLECT_H
#include "g2048.h"
#ifdef __cplusplus
extern "C" {
#endif

#define G2048_TPOLICY_COLLECT_ABI_VERSION 1

/* opts of g2048_tpolicy_collect, the bits of g2048_ppo_collect's (g2048_ppo_collect.h): G2048_STEP_REWARD_F64 (reward_out is
 * double), the dtype of obs_out as G2048_OBS_F32 / F16 / BF16 << G2048_ROLLOUT_OBS_SHIFT, and the blob's precision,
 * G2048_POLICY_F32 / BF16 << G2048_TPOLICY_COLLECT_PRECISION_SHIFT. G2048_STEP_AUTO_RESET is always in force and may be set. */
#define G2048_TPOLICY_COLLECT_PRECISION_SHIFT 8

G2048_API const char *g2048_tpolicy_collect_last_error(void);
G2048_API int g2048_tpolicy_collect_abi_version(void);

/* Arrays are [steps][n] unless stated otherwise. For t = 0 .. steps - 1 and environment i, with index = step_index0 +
 * (*step_counter_or_null if given) + t and id = env_id_base + i, every line is bit for bit what the named entry point of g2048.h
 * gives:
 *   probabilities  g2048_tpolicy_forward of the environment's current board with `packed` (the blob of g2048_tpolicy_pack for
 *                  dim_ff, n_layers and the precision in opts); value_out[t][i] that call's value, written when value_out is
 *                  given. The value does not feed the action.
 *   step           actions_out, prob_out (the probability, not its log), reward_out (float, or double under
 *                  G2048_STEP_REWARD_F64), flags_out, next_boards_out (16 bytes a board, BEFORE any reset) and
 *                  state_maxcode_out (the max code of the board acted in): g2048_rollout_step with G2048_STEP_AUTO_RESET and
 *                  mask4_in NULL, i.e. the draws (seed, POLICY, index, id), (seed, STEP, index, id) and the two EPISODE draws
 *                  of that index and id. A board with no valid move is sampled among all four actions.
 *   rows           obs_out [steps + 1][n][16] (dtype by the OBS bits) and mask4_out [steps + 1][n]: row t + 1 is the
 *                  observation (g2048_obs_f32 / g2048_obs_16) and the env valid-move mask (g2048_valid_moves) of the board
 *                  the environment goes on from -- the next board, or the fresh board after a DONE; row 0 the same for the
 *                  boards the call starts from.
 * After the last step boards_inout (16 bytes a board) and score_inout hold the environments' state (score 0 after a reset).
 * No episode cap. ONE kernel launch and nothing else on the stream: no workspace, no atomics, no block waits on another; two
 * calls give the same bits. step_counter_or_null is read on the device, so a captured call replays with the counter's value of
 * the time, and `packed` is read by the launch, so a blob packed in place acts in the next call or replay. Nothing outside the
 * stated extents is written. dim_ff: a multiple of 32 (32 .. 65536); n_layers 1 .. 64.
 * Alignment: boards, next boards, blob, obs: 16 bytes; reward, counter: 8 under their 64-bit forms; score, prob, value: 4. */
G2048_API int g2048_tpolicy_collect(void *boards_inout, uint32_t *score_inout, const void *packed, int dim_ff, int n_layers,
                                    uint8_t *actions_out, float *prob_out, void *reward_out, uint8_t *flags_out, float *value_out_or_null,
                                    void *obs_out_or_null, uint8_t *mask4_out_or_null, void *next_boards_out_or_null,
                                    uint8_t *state_maxcode_out_or_null, uint64_t seed, uint64_t step_index0,
                                    const unsigned long long *step_counter_or_null, uint64_t env_id_base, size_t n, int steps,
                                    uint32_t opts, void *stream);

#ifdef __cplusplus
}
#endif
#endif
