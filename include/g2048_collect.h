/*
 * g2048_collect.h -- the C-ABI of libg2048_collect_hip.so: the hybrid agent's experience collection (the acting half of
 * train_agent, agents/hybrid.py:1098-1127) in one kernel launch. `steps` moves of `n` environments are played with the
 * Q-network and DQNAgent.select_action, and every transition goes straight into the prioritized replay ring of g2048.h
 * ("prioritized experience replay"). A small library next to libg2048_hip.so (include/g2048.h), built from
 * csrc/g2048_qnet_collect.hip; it has its own error string and version, and needs nothing of the main library at run time. The
 * conventions are g2048.h's: device pointers, `stream` a hipStream_t (NULL: the default stream), G2048_OK or an error code with a
 * message in g2048_collect_last_error() (per thread), argument checks before any device call, n == 0 returns G2048_OK and does
 * nothing.
 */
#ifndef G2048_COLLECT_H
#define G2048_COLLECT_H
#include "g2048.h"
#ifdef __cplusplus
extern "C" {
#endif

#define G2048_COLLECT_ABI_VERSION 1

G2048_API const char *g2048_collect_last_error(void);
G2048_API int g2048_collect_abi_version(void);

/* Bytes of the workspace g2048_qnet_collect needs for n environments (the ring's priority maximum, padded). */
G2048_API size_t g2048_qnet_collect_workspace(size_t n);

/* For t = 0 .. steps - 1, environment i (id env_id_base + i, step index step_index0 + t), every line bit for bit what the named
 * entry point of g2048.h gives:
 *   Q-values   g2048_qnet_forward of the environment's board with `packed` (the blob of g2048_qnet_pack for opts = G2048_POLICY_F32
 *              or G2048_POLICY_BF16, dim_ff, n_layers).
 *   action     beam_width == 0 (use_beam_search False): g2048_qnet_select_actions at `epsilon` (epsilon 0 makes no draw);
 *              beam_width 1 .. 64: g2048_qnet_beam_actions at (beam_width, search_depth, threshold). search_depth 1 is refused, as
 *              g2048_play_qnet_beam_games refuses it; without the beam search_depth and threshold are not read.
 *   env step   g2048_step without options: the next board, the float32 reward and the flags byte.
 *   ring       transition k = t n + i lands where g2048_per_push puts entry k of a push of steps x n rows: slot
 *              (head + size + k) % capacity holds the board before the move, the next board BEFORE any reset, the action, the
 *              reward, done = flags & 1 and the priority M = the maximum of the `size` live priorities before the call (1.0 for an
 *              empty ring). steps x n must not exceed capacity. The caller updates size and head as for such a push.
 *   episode    moves_inout[i] counts the episode's moves. When the step set DONE, or max_episode_steps > 0 and the count reached it
 *              (train_agent's `step < max_steps`; the stored done stays 0 then), the environment goes on from the board g2048_step
 *              with G2048_STEP_AUTO_RESET writes for a finished board -- fresh_board of the two EPISODE-domain draws of that step
 *              index and id -- with score 0 and count 0.
 *   flags      flags_stream_out_or_null[t n + i] = the step's flags byte.
 * After the last step boards_inout (16 bytes a board), score_inout and moves_inout hold the environments' state. One kernel
 * launch, after a memset and one small launch for M when size > 0: at most three stream operations. Nothing outside the stated
 * extents is written. workspace: g2048_qnet_collect_workspace(n) bytes, 4-byte aligned. */
G2048_API int g2048_qnet_collect(void *boards_inout, uint32_t *score_inout, int32_t *moves_inout, const void *packed, int dim_ff,
                                 int n_layers, uint32_t opts, float epsilon, int beam_width, int search_depth, int threshold, uint64_t seed,
                                 uint64_t step_index0, uint64_t env_id_base, size_t n, int steps, int max_episode_steps, void *states,
                                 void *next_states, uint8_t *actions, float *rewards, uint8_t *dones, float *priorities, size_t capacity,
                                 size_t size, size_t head, uint8_t *flags_stream_out_or_null, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif
