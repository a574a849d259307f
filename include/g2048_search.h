/*
 * g2048_search.h -- the C-ABI of libg2048_search_hip.so: the expectimax agent. Where g2048_beam_get_action (g2048.h) samples one
 * spawn per node and ranks by a heuristic, this search takes the expectation over ALL spawn successors (tile 2 with probability
 * 0.9, tile 4 with 0.1) and the maximum over the valid moves, 1 to 3 plies deep, with the beam agent's leaf heuristic. A small
 * library next to libg2048_hip.so (include/g2048.h), built from csrc/g2048_expectimax.hip; it has its own error string and
 * version, and needs nothing of the main library at run time. The conventions are g2048.h's: device pointers, `stream` a
 * hipStream_t (NULL: the default stream), G2048_OK or an error code with a message in g2048_search_last_error() (per thread),
 * argument checks before any device call, n == 0 returns G2048_OK and does nothing.
 *
 * The function, exactly (everything f64 with separate multiplies and adds, never fma; moves are the env's, Game2048Env.
 * _execute_move, actions 0 LEFT, 1 UP, 2 RIGHT, 3 DOWN -- not BeamSearchAgent._make_move with its rot180 DOWN):
 *   leaf(B) = BeamSearchAgent._evaluate_state(B) in the phase of B's own max tile (early below early_thr, mid below mid_thr,
 *             late from there on: g2048_eval kind G2048_EVAL_FULL with that phase; the thresholds are tile values, 512 and 1024 in
 *             the reference)
 *   V(B, 0) = leaf(B)
 *   V(B, d) = leaf(B) if no move is valid, else the maximum over the valid actions a, ascending, of C(move(B, a), d)
 *   C(M, d) = acc / (double)e, e = the number of empty cells of M, acc = 0.0 and then, for each empty cell c in row-major order,
 *             acc += 0.9 * V(M + 2@c, d - 1) + 0.1 * V(M + 4@c, d - 1) (both products first, then their sum, then the addition)
 * The decision for a board is the action with the largest C(move(B, a), depth) among the env's valid moves that the caller's mask
 * allows, ties to the lowest action; 0 if none is left. The sums are taken in this order whatever the launch geometry, so a CPU
 * restatement of these lines agrees bit for bit.
 */
#ifndef G2048_SEARCH_H
#define G2048_SEARCH_H
#include "g2048.h"
#ifdef __cplusplus
extern "C" {
#endif

#define G2048_SEARCH_ABI_VERSION 1
#define G2048_EXPECTIMAX_MAX_DEPTH 3

G2048_API const char *g2048_search_last_error(void);
G2048_API int g2048_search_abi_version(void);

/* One decision per board. boards: n x 16 bytes (g2048.h's codes). mask4_or_null[i]: bit a set = action a may be chosen (ANDed
 * with the env's valid moves; NULL: all four). actions_out[i]: the decision. values_out_or_null: n x 4 doubles, the four
 * C(move(B, a), depth), -inf for an action that is invalid or masked out. depth: 1 .. G2048_EXPECTIMAX_MAX_DEPTH.
 * ONE kernel launch, one wavefront per board, no workspace, no atomics; two calls give the same bits. Nothing outside the stated
 * extents is written. Alignment: boards 16 bytes, values 8. */
G2048_API int g2048_expectimax_actions(const void *boards, const uint8_t *mask4_or_null, uint8_t *actions_out, double *values_out_or_null,
                                       int depth, int early_thr, int mid_thr, size_t n, void *stream);

/* Complete games of the agent, every game played to the end on the device in ONE launch, as g2048_play_policy_games (g2048.h)
 * plays a network's: game g (global id game_id_base + g) starts from boards_inout[g] / score_inout[g]; at move t = 0, 1, ... its
 * action is g2048_expectimax_actions' for the board (no mask), and the board is stepped exactly as g2048_step(step_index = t,
 * board id = game id) does, without auto-reset. The game ends when it is over (DONE) or after max_moves moves. The outputs, the
 * workspace (g2048_play_expectimax_workspace(n_games) bytes, 8-byte aligned: a ticket counter the call clears on `stream`) and
 * the alignments are g2048_play_policy_games'. max_waves = the number of wavefronts, one game in flight each (a finished game's
 * wavefront takes the next game), 0 = as many as the chip holds at once; the games do not depend on it. Nothing past game
 * n_games is written. */
G2048_API size_t g2048_play_expectimax_workspace(size_t n_games);
G2048_API int g2048_play_expectimax_games(void *boards_inout, uint32_t *score_inout, int depth, int early_thr, int mid_thr, int32_t *moves_out,
                                          int32_t *valid_out, int32_t *invalid_out, int32_t *milestone_move_out, double *reward_sum_out_or_null,
                                          uint8_t *alive_out, uint8_t *actions_out_or_null, int max_moves, uint64_t seed, uint64_t game_id_base,
                                          size_t n_games, uint32_t max_waves, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
