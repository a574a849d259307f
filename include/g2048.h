/*
 * g2048.h -- C-ABI of the MI355X (gfx950) batched 2048 rollout / beam-search engine.
 *
 * The reference (vivek-tiwari-vt/2048-Using-Reinforcement-Learning) has NO FFI,
 * plugin or operator interface: its boundary is two Python classes. This header
 * is therefore the boundary the build defines for that hot path; each entry
 * point names the reference method it replaces (file:line, relative to the
 * reference root). INTEGRATION.md shows the ctypes binding a maintainer of the
 * reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into caller-owned memory (e.g. a
 *     torch.Tensor's data_ptr()); scratch is caller-provided too (the *_ws entry
 *     points with their *_workspace queries). ONE entry point allocates:
 *     g2048_play_games, the convenience form of g2048_play_games_ws, takes its
 *     helper workspace from the stream-ordered pool (hipMallocAsync / hipFreeAsync
 *     on `stream`). Nothing ever synchronises: work is enqueued on `stream` (a
 *     hipStream_t passed as void*, NULL = the default stream) and is stream-ordered;
 *   - a board is 16 bytes: 16 x uint8 log2 codes, row-major (0 = empty,
 *     1 = tile 2, ... 17 = tile 131072). Board arrays must be 16-byte aligned;
 *   - return value: 0 = G2048_OK, negative = error (g2048_last_error() gives
 *     the text for the calling thread). Nothing throws, nothing prints;
 *   - randomness is a counter RNG keyed by (seed, domain, step/epoch index,
 *     GLOBAL board id, counter): results do not depend on launch geometry or
 *     on how boards are sharded over GPUs (DESIGN.md "RNG");
 *   - thread-safe: no global mutable state apart from the thread-local error
 *     string; no environment variable is read (round 2's G2048_PLAY_TUNE hook is
 *     gone: g2048_play_games_tuned takes the same numbers as an argument);
 *   - launch geometry that depends on the chip's size (how many helper wavefronts a
 *     launch may carry, how a beam batch is dealt to the SIMDs) is derived per call
 *     from the compute-unit count of the current device (g2048_launch_plan shows
 *     the arithmetic).
 * There is no CPU implementation behind this ABI: without a HIP device every
 * compute entry point fails with G2048_ERR_HIP.
 */
#ifndef G2048_H
#define G2048_H
#include <stddef.h>
#include <stdint.h>
/* Every entry point below is exported (the library is built with -fvisibility=hidden: nothing else is). */
#ifndef G2048_API
#define G2048_API __attribute__((visibility("default")))
#endif
#ifdef __cplusplus
extern "C" {
#endif

#define G2048_ABI_VERSION 5        /* 5: round 5, second half (ops MOVE / SPAWN / MOVE_AGENT of g2048_env_step; g2048_eval kinds CORNER_BONUS and
                                      MERGE_POTENTIAL; no entry point added or removed;
                                      later, additive: g2048_policy_packed_bytes / _pack / _forward,
                                      g2048_play_policy_games / _workspace, g2048_tpolicy_packed_bytes / _pack / _forward,
                                      g2048_play_tpolicy_games / _workspace, g2048_qnet_packed_bytes / _pack / _forward,
                                      g2048_qnet_select_actions, g2048_play_qnet_games / _workspace, g2048_qnet_beam_actions / _expand,
                                      g2048_play_qnet_beam_games / _workspace, g2048_per_push / _sample / _sample_workspace /
                                      _update_priorities / _update_workspace, g2048_dqn_shape_rewards, g2048_qnet_forward_batch,
                                      g2048_qnet_batch_workspace, g2048_dqn_targets, g2048_qnet_loss_grad / _grad_workspace,
                                      g2048_qnet_adamw_step / _step_workspace, g2048_ppo_train_workspace / _forward_train /
                                      _advantages / _loss_grad, g2048_ppo_adam_step / _step_workspace,
                                      g2048_ppo_forward_train_dropout / _loss_grad_dropout / g2048_ppo_dropout_mask)
                                      4: round 5 (export table = this header + g2048_testing.h exactly: test / measurement hooks moved there,
                                      internal symbols hidden; g2048_replay_games also clamps a game's length to actions_stride)
                                      3: round 4 (actions_out of the g2048_play_games family, g2048_replay_games, g2048_env_step,
                                      g2048_minibatch_gather, g2048_build_flags; the A/B variants of g2048_step / g2048_sort_selftest gone)
                                      2: round 3 (g2048_step_many, g2048_play_games_tuned, g2048_launch_plan, g2048_device_plan,
                                      g2048_beam_get_action_hist; no env hook) */

enum {
    G2048_OK = 0,
    G2048_ERR_ARG = -1,        /* bad argument (null pointer, misaligned board array, bad enum) */
    G2048_ERR_HIP = -2         /* HIP runtime error (no device, launch failure) */
};

/* flags_out byte of g2048_step */
#define G2048_FLAG_DONE        0x01u   /* game over after this step (game_2048.py:198, :279-288) */
#define G2048_FLAG_VALID       0x02u   /* the move changed the board (game_2048.py:188)          */
#define G2048_FLAG_MAXCODE_SHIFT 3     /* bits 3..7: max log2 code after the step -> info["highest_tile"] */

/* opts of g2048_step */
#define G2048_STEP_REWARD_F64  0x01u   /* reward_out is double[n] (parity mode); default float[n] = (float)f64 reward */
#define G2048_STEP_AUTO_RESET  0x02u   /* finished boards are replaced by a fresh episode (score 0); flags keep DONE */
#define G2048_STEP_RANDOM_ACTIONS 0x04u /* random playouts: `actions` is ignored (may be NULL); board i moves in direction
                                          draw(seed, SYNTH_ACTION, step_index, id) >> 30, exactly what g2048_synth_actions
                                          writes for the same (seed, step_index, id) */

#define G2048_STEP_NOOP_ACTIONS 0x08u  /* an action byte above 3 moves nothing -- an invalid move -- exactly as the reference's
                                          _execute_move (game_2048.py:97-114) treats values other than 0..3; without this
                                          flag only the low two bits of the byte are looked at */

/* tuning only (results identical): bits 8..9 pick the boards-per-lane variant: 0 = library default (one board per lane, two
 * from 4 Mi boards per launch on), 1 = one, 2 = two */
#define G2048_STEP_TUNE_SHIFT  8

/* opts of g2048_valid_moves */
#define G2048_VALID_ENV        0x00u   /* Game2048Env.get_valid_moves semantics (game_2048.py:69-95) */
#define G2048_VALID_AGENT      0x01u   /* BeamSearchAgent._check_valid_moves semantics, incl. its DOWN quirk
                                          (beam_search_agent.py:183-192, :209-210 vs :251-253) */

/* kind of g2048_eval */
enum {
    G2048_EVAL_FAST = 0,       /* BeamSearchAgent._fast_evaluate   beam_search_agent.py:280-314 */
    G2048_EVAL_FULL = 1,       /* BeamSearchAgent._evaluate_state  beam_search_agent.py:316-403 (phase per board) */
    G2048_EVAL_PPO_HEURISTIC = 2, /* PPOAgent.evaluate_heuristic   ppo_agent.py:271-298 */
    G2048_EVAL_MONO_PP = 3,    /* PPOAgent.monotonicity(board, +1, +1)  ppo_agent.py:300-333 */
    G2048_EVAL_MONO_PM = 4,    /*                        (+1, -1) */
    G2048_EVAL_MONO_MP = 5,    /*                        (-1, +1) */
    G2048_EVAL_MONO_MM = 6,    /*                        (-1, -1) */
    G2048_EVAL_PPO_SHAPING = 7,/* the pure per-transition terms of PPOAgent.remember, ppo_agent.py:253-266:
                                  0.1 * sum(log2(top-4 tiles)) + 0.3 * evaluate_heuristic (stateful terms excluded) */
    G2048_EVAL_PATTERN = 8,    /* Game2048Env._evaluate_pattern  game_2048.py:313-339 (snake / corner weights on tile values) */
    G2048_EVAL_CORNER_BONUS = 9,     /* BeamSearchAgent._calculate_corner_bonus     beam_search_agent.py:375-385 (unweighted) */
    G2048_EVAL_MERGE_POTENTIAL = 10  /* BeamSearchAgent._calculate_merge_potential  beam_search_agent.py:387-403 (unweighted) */
};

/* opts of g2048_beam_get_action */
#define G2048_BEAM_FIXED_DOWN  0x01u   /* use the true DOWN move instead of the reference's rot180 quirk (not parity) */

#define G2048_BEAM_RANK_BY_COUNTING 0x04u /* rank every level by the counting loop instead of the sorting network (same
                                              decisions; an A/B switch for tests and measurements; also g2048_play_games) */
/* further opts of g2048_play_games */
#define G2048_PLAY_ONE_PHASE   0x02u   /* every game on its one wavefront only, no speculative helper wavefronts; the games
                                          are the same either way -- an A/B switch for tests and measurements */

#define G2048_BEAM_MAX_WIDTH   128

G2048_API const char *g2048_last_error(void);
G2048_API int g2048_abi_version(void);
/* 0 for the product library. Non-zero: a measurement build (csrc/g2048_instrument.h: bit 0 beam timeline, bit 1 evaluation
 * timeline, bit 2 step timeline) that overwrites real outputs with clock ticks -- never use its results. */
G2048_API unsigned g2048_build_flags(void);
/* number of visible HIP devices (0 on a CPU-only host); never fails */
G2048_API int g2048_device_count(void);

/* Game2048Env.step for n boards (environment/game_2048.py:170-210): move, validity, spawn iff valid,
 * shaped reward (:212-277), done (:279-288). boards_out may alias boards_in. Draw for board i:
 * (seed, STEP, step_index, board_id_base + i). */
G2048_API int g2048_step(const void *boards_in, const uint8_t *actions, void *boards_out,
               uint32_t *score_inout, void *reward_out, uint8_t *flags_out,
               uint64_t seed, uint64_t step_index, uint64_t board_id_base, size_t n,
               uint32_t opts, void *stream);

/* g2048_step for a caller that makes the same call step after step (a host-paced loop of launches): everything but the step
 * index and the stream is checked and bound ONCE, into a caller-owned block, and each step is then a call of three arguments.
 *   g2048_step_pack    performs every argument check of g2048_step (null pointers, alignment, unknown opts, tune 3) and fills
 *                      call_out -- G2048_STEP_CALL_BYTES bytes, 8-byte aligned -- with the bound arguments, the kernel variant
 *                      and grid g2048_step would choose, and a magic word. It makes no HIP call. It refuses, with
 *                      G2048_ERR_ARG, what is not one plain launch: G2048_STEP_RANDOM_ACTIONS, G2048_STEP_NOOP_ACTIONS and a
 *                      range of board ids that crosses a multiple of 2^32; such a caller keeps using g2048_step. A refused
 *                      call leaves a block g2048_step_packed does not accept.
 *   g2048_step_packed  derives the keys of step_index and makes exactly the launch g2048_step(..., step_index, ..., stream)
 *                      would make with the bound arguments: the results are the same bit for bit. A block without the magic
 *                      word is refused with G2048_ERR_ARG. The block may be copied and reused for any number of calls, on any
 *                      stream; the arrays it names must be alive at every call. */
#define G2048_STEP_CALL_BYTES 128
G2048_API int g2048_step_pack(const void *boards_in, const uint8_t *actions, void *boards_out,
               uint32_t *score_inout, void *reward_out, uint8_t *flags_out,
               uint64_t seed, uint64_t board_id_base, size_t n, uint32_t opts, void *call_out);
G2048_API int g2048_step_packed(const void *call, uint64_t step_index, void *stream);

/* `steps` consecutive Game2048Env.step calls (environment/game_2048.py:170-210) of every board in ONE launch: the board and
 * its score stay in registers between the steps instead of making a 46-byte round trip through memory per step. Step t
 * (0 <= t < steps) is bit-for-bit g2048_step(step_index = step_index0 + t) with the same opts. The actions are either the
 * in-kernel uniform draws (G2048_STEP_RANDOM_ACTIONS: random playouts, SURVEY 8d C2 "rollout" variant; actions_stream_or_null
 * is ignored and may be NULL) or explicit, step-major: actions_stream_or_null[t * n + i] (low two bits, as in g2048_step) --
 * a recorded move sequence such as the reference's checkpoints/ move-set files (BeamSearchAgent_best_moveset_tile_N.txt), or an open-loop plan; a policy that needs the
 * state of step t to choose action t uses g2048_step / g2048_rollout_step. G2048_STEP_AUTO_RESET and G2048_STEP_REWARD_F64
 * are optional. boards_out may alias boards_in.
 * Outputs: the boards and scores after the last step, flags_last_out[i] = the flags byte of the last step; optional per-step
 * streams, step-major: reward_stream_out_or_null[t * n + i] (float, or double with G2048_STEP_REWARD_F64) and
 * flags_stream_out_or_null[t * n + i]; episodes_out_or_null[i] = episodes board i finished (auto-resets taken). */
G2048_API int g2048_step_many(const void *boards_in, const uint8_t *actions_stream_or_null, void *boards_out, uint32_t *score_inout,
                    void *reward_stream_out_or_null, uint8_t *flags_stream_out_or_null, uint8_t *flags_last_out,
                    uint32_t *episodes_out_or_null, uint64_t seed, uint64_t step_index0, uint32_t steps,
                    uint64_t board_id_base, size_t n, uint32_t opts, void *stream);

/* Game2048Env.reset for n boards (environment/game_2048.py:29-48). score_out may be NULL. */
G2048_API int g2048_reset(void *boards_out, uint32_t *score_out, uint64_t seed, uint64_t epoch,
                uint64_t board_id_base, size_t n, void *stream);

/* get_valid_moves / _check_valid_moves: mask4_out[i] bit a = action a valid (0 LEFT 1 UP 2 RIGHT 3 DOWN). */
G2048_API int g2048_valid_moves(const void *boards, uint8_t *mask4_out, size_t n, uint32_t opts, void *stream);

/* board heuristics, f64 out. phase_or_null: per-board 0 early / 1 mid / 2 late for G2048_EVAL_FULL
 * (NULL = derive from the board's own max tile with thresholds 512 / 1024, beam_search_agent.py:271-278). */
G2048_API int g2048_eval(const void *boards, int kind, const uint8_t *phase_or_null, double *out, size_t n, void *stream);

/* PPOAgent.normalize_state (agents/ppo_agent.py:184-195): obs_out[i*16+j] = float32(code)/float32(15). */
G2048_API int g2048_obs_f32(const void *boards, float *obs_out, size_t n, void *stream);

/* the same observation in 16 bits: obs_out is n*16 IEEE half (bf16 = 0) or bfloat16 (bf16 = 1) values, each the f32
 * quotient above rounded to nearest even -- for policies that run in reduced precision (32 B per board instead of 64) */
G2048_API int g2048_obs_16(const void *boards, void *obs_out, int bf16, size_t n, void *stream);

/* BeamSearchAgent.get_action for n_games roots (agents/beam_search_agent.py:71-181).
 * valid_mask_or_null: caller-supplied masks (the `valid_moves` argument), NULL = None.
 * expanded_out_or_null: children generated per game (calls of _add_random_tile).
 * Draw j of game g: (seed, BEAM, step_index, game_id_base + g, j) in the reference's generation order. */
G2048_API int g2048_beam_get_action(const void *root_boards, const uint8_t *valid_mask_or_null,
                          uint8_t *action_out, float *prob_out, uint32_t *expanded_out_or_null,
                          int width, int depth, int early_threshold, int mid_threshold,
                          uint64_t seed, uint64_t step_index, uint64_t game_id_base, size_t n_games,
                          uint32_t opts, void *stream);
/* The same with g2048_beam_workspace_bytes(n_games) bytes of caller-provided device scratch: from 4096 games per
 * call on, the blocks then take the games in a depth-balanced order (deep and shallow searches mixed on every SIMD) -- same
 * results, a shorter launch. workspace NULL, or a batch for which the query returns 0: exactly g2048_beam_get_action. */
G2048_API size_t g2048_beam_workspace_bytes(size_t n_games);
G2048_API int g2048_beam_get_action_ws(const void *root_boards, const uint8_t *valid_mask_or_null, uint8_t *action_out,
                             float *prob_out, uint32_t *expanded_out_or_null, int width, int depth,
                             int early_threshold, int mid_threshold, uint64_t seed, uint64_t step_index,
                             uint64_t game_id_base, size_t n_games, uint32_t opts, void *workspace,
                             size_t workspace_bytes, void *stream);
/* The same order without its own launch, for callers that search batch after batch (an evaluation loop): every block of a
 * call files its game into per-class lists in `history`, and the NEXT call deals the games from them -- the balanced order of
 * the previous batch's roots (any order gives the same results; this one is balanced as far as a game keeps its depth class
 * from one call to the next). history: g2048_beam_history_bytes(n_games) bytes of device memory, ZERO-FILLED before its first
 * use and again whenever a call is not the direct successor (call_index + 1, same n_games, same buffer, stream-ordered after
 * it) of the last call that used it; call_index counts 1, 2, 3, ... . A call that finds no usable history takes the games in
 * caller order. history NULL, or a batch for which the query returns 0: exactly g2048_beam_get_action. One buffer serves one
 * stream of calls; it must not be shared by calls that may run concurrently. */
G2048_API size_t g2048_beam_history_bytes(size_t n_games);
G2048_API int g2048_beam_get_action_hist(const void *root_boards, const uint8_t *valid_mask_or_null, uint8_t *action_out,
                               float *prob_out, uint32_t *expanded_out_or_null, int width, int depth,
                               int early_threshold, int mid_threshold, uint64_t seed, uint64_t step_index,
                               uint64_t game_id_base, size_t n_games, uint32_t opts, void *history, size_t history_bytes,
                               uint32_t call_index, void *stream);

/* Per-move bookkeeping of the reference's evaluation loops (evaluate_beam_search.py:42-64, run_evaluation.py:56-69)
 * for n games after a g2048_step: for games still alive, milestone_move_inout[i][k] (k = 0..7 for tiles 64..8192,
 * -1 = not reached yet) records move_index the first time the max tile reaches it, the valid / invalid / total move
 * counters advance, expanded_or_null[i] is added to expanded_sum, and the game leaves `alive` when its DONE flag is
 * set. Games not alive are untouched. */
G2048_API int g2048_track_episodes(const uint8_t *flags, const uint32_t *expanded_or_null, uint8_t *alive_inout, int32_t *moves_inout,
                         int32_t *valid_inout, int32_t *invalid_inout, int32_t *milestone_move_inout,
                         unsigned long long *expanded_sum_inout_or_null, int32_t move_index, size_t n, void *stream);

/* The masked sampling of PPOAgent.get_action (agents/ppo_agent.py:211-221) for n envs: probs is float32 [n][4]
 * (the actor's softmax output), mask4 as g2048_valid_moves writes it (NULL = all valid). The action is drawn from
 * weights p_a + 1e-10 over the valid actions (what Categorical(logits = log(p + 1e-10) + mask) samples) by inverse
 * CDF with draw (seed, POLICY, step_index, env_id_base + i); prob_out[i] = its probability (take the log for
 * the reference's `action_prob`). */
G2048_API int g2048_sample_actions(const float *probs, const uint8_t *mask4_or_null, uint8_t *actions_out, float *prob_out,
                         uint64_t seed, uint64_t step_index, uint64_t env_id_base, size_t n, void *stream);

/* Game2048Env.simulate_move (environment/game_2048.py:341-387) for n (state, action) pairs: every successor the
 * reference lists -- 2 per empty cell of the moved board, at most 30 -- in its order and with its behaviour (each
 * successor is built on top of the previous one; its reward is computed on the previous successor's board and
 * includes the milestone bonus against highest_code, the env's highest_tile attribute as a log2 code; NULL = the
 * state's own max, as inside an episode). Outputs are 32 slots per state: succ_boards_out n*32 boards,
 * reward_out n*32 f64, done_out n*32 bytes; count_out[i] = number of valid slots (0 when the move is invalid). */
G2048_API int g2048_simulate_move(const void *boards, const uint8_t *actions, const uint8_t *highest_code_or_null,
                        void *succ_boards_out, double *reward_out, uint8_t *done_out, uint8_t *count_out,
                        size_t n, void *stream);

/* The hybrid agent's simulate_move (agents/hybrid.py:578-629, the function it monkey-patches onto its own copy of the
 * env, :694-697) for n (state, action) pairs: the move, then up to three distinct empty cells of the moved board
 * (random.sample), each as a 2-successor and a 4-successor whose reward (_calculate_simulation_reward, :671-692) is
 * weighted by 0.9 / 0.1. Outputs are 8 slots per state: succ_boards_out n*8 boards, reward_out n*8 f64, done_out n*8
 * bytes; count_out[i] = valid slots: 1 for a move that changes nothing (the board itself, reward -1.0), else 2 * min(3,
 * empty cells), successor 2j / 2j+1 = pick j with a 2 / a 4. Pick j of state i is the idx(h_j, n_empty - j)-th empty
 * cell (row-major) not picked before, h_j = draw (seed, SIMULATE, step_index, state_id_base + i, j). */
G2048_API int g2048_simulate_move_sampled(const void *boards, const uint8_t *actions, void *succ_boards_out, double *reward_out,
                                uint8_t *done_out, uint8_t *count_out, uint64_t seed, uint64_t step_index,
                                uint64_t state_id_base, size_t n, void *stream);

/* The reference's evaluation loop (run_evaluation.py:48-69, evaluate_beam_search.py:16-98) fused per game: every game
 * (one wavefront) alternates BeamSearchAgent.get_action (no caller mask) and Game2048Env.step from boards_inout /
 * score_inout until it is over or max_moves is reached, entirely on the device. Move t of game g uses the draws of
 * g2048_beam_get_action(step_index = t, game id g) and g2048_step(step_index = t, board id g), so the outcome equals
 * the step-by-step loop. Unless opts has G2048_PLAY_ONE_PHASE (or n_games > 65,536) the launch also carries helper
 * wavefronts that search the roots a game's next moves can start from ahead of time (same decisions, less latency for the
 * last games). They need g2048_play_games_workspace(n_games) bytes of device scratch: g2048_play_games_ws takes it from
 * the caller (64-byte aligned; NULL = play without helpers), g2048_play_games from hipMallocAsync on `stream`.
 * Outputs per game: final board / score (in place), moves played, valid / invalid move counts,
 * milestone_move_out[g][0..8) = move at which tiles 64..8192 first appeared (-1 = never), total children expanded
 * (optional), alive_out[g] = 1 if the game hit max_moves without finishing.
 * actions_out_or_null (ABI 3): the move-set of every game -- what train.py:51,67 collects in `moveset` and :140-142 writes to
 * *_best_moveset_tile_N.txt --, n_games rows of max_moves bytes: actions_out[g * max_moves + t] = the action of move t (0..3),
 * 0xFF from the game's end on (the library fills the array with 0xFF before the launch). One byte per move is also all that is
 * needed to rebuild the per-move histories of evaluate_beam_search.py:44-50, :72-75 afterwards: g2048_replay_games. The bytes do
 * not depend on helper wavefronts, tuning or the ranking switch. */
G2048_API int g2048_play_games(void *boards_inout, uint32_t *score_inout, int32_t *moves_out, int32_t *valid_out,
                     int32_t *invalid_out, int32_t *milestone_move_out, unsigned long long *expanded_sum_out_or_null,
                     uint8_t *alive_out, uint8_t *actions_out_or_null, int width, int depth, int early_threshold,
                     int mid_threshold, int max_moves, uint64_t seed, uint64_t game_id_base, size_t n_games, uint32_t opts,
                     void *stream);
G2048_API size_t g2048_play_games_workspace(size_t n_games);
G2048_API int g2048_play_games_ws(void *boards_inout, uint32_t *score_inout, int32_t *moves_out, int32_t *valid_out,
                        int32_t *invalid_out, int32_t *milestone_move_out, unsigned long long *expanded_sum_out_or_null,
                        uint8_t *alive_out, uint8_t *actions_out_or_null, int width, int depth, int early_threshold,
                        int mid_threshold, int max_moves, uint64_t seed, uint64_t game_id_base, size_t n_games, uint32_t opts,
                        void *workspace, size_t workspace_bytes, void *stream);

/* Recorded games replayed into the per-move histories of the reference's run_game (evaluate_beam_search.py:44-50, :72-75,
 * :88-97: board_history, max_tiles_history, scores_history; :185-196 game_N_data.json): game k starts from boards0[k] with score
 * score0_or_null[k] (NULL: 0) and plays actions[k * actions_stride + t], t = 0 .. n_moves[k] - 1, with the draw of
 * g2048_step(step_index = t, board id = game_ids_or_null[k], or game_id_base + k) -- exactly the moves g2048_play_games made
 * when it wrote those bytes; an action byte above 3 (0xFF = no move) ends that game's replay early. Outputs, hist_stride
 * entries per game (hist_stride > the longest game): boards_hist_out[k * hist_stride + t] = the board BEFORE move t (t = 0 the
 * start, t = n_moves[k] the final board), score_hist_out likewise, flags_hist_out[k * hist_stride + t] = the flags byte of move
 * t (DONE / VALID / max code after the move: bits 3..7 give max_tiles_history). Entries past a game's end are left untouched.
 * A game's length is clamped to min(n_moves[k], hist_stride - 1, actions_stride): the kernel never reads past a game's row of
 * action bytes nor writes past its row of the history; actions_stride = 0 or hist_stride = 0 is refused. */
G2048_API int g2048_replay_games(const void *boards0, const uint32_t *score0_or_null, const uint64_t *game_ids_or_null, uint64_t game_id_base,
                       const uint8_t *actions, size_t actions_stride, const int32_t *n_moves, void *boards_hist_out,
                       uint32_t *score_hist_out_or_null, uint8_t *flags_hist_out_or_null, size_t hist_stride, uint64_t seed,
                       size_t n, void *stream);

/* ONE env driven from a host loop -- the drop-in Game2048Env of train.py:55-75 -- in one launch per iteration: op STEP =
 * Game2048Env.step(action) (environment/game_2048.py:170-210; an action outside 0..3 moves nothing, :97-114; draw (seed, STEP,
 * index, board_id)), op RESET = Game2048Env.reset() (:29-48; draws (seed, RESET, index, board_id)), op PEEK = nothing moves.
 * board_inout (16 bytes) / score_inout are updated in place, and record_out -- G2048_ENV_RECORD_BYTES bytes of device memory or
 * of pinned, device-visible host memory, 16-byte aligned -- receives everything the host mirrors of the env need, so that an
 * iteration costs one launch and one copy: [0,64) the state as int32 tile values (get_state, :50-57), [64,68) int32 score,
 * [68] the flags byte (DONE / VALID / max code), [69] the valid-move mask of the NEW state (get_valid_moves, :69-95, for the
 * next iteration), [70,72) a 16-bit token, [72,80) the f64 reward (:212-277; 0.0 for every op but STEP). The token is bits
 * 8..23 of `op` (G2048_ENV_TOKEN_SHIFT; 0 if the caller passes a bare op) and is written LAST, behind a system-scope fence: a host
 * that passes a fresh non-zero token and polls [70,72) of a pinned record has the complete record when it reads the token back
 * -- no stream synchronisation in the loop (the drop-in Game2048Env does this: ~2x the iterations per second).
 * The pieces of a step as ops of their own (the reference's methods of the same names, for callers that drive them directly):
 * op MOVE = Game2048Env._execute_move(action) (:97-114; action 0 is _move_left, :116-168): the slide / merge alone -- score +=
 * merged tiles, no spawn; flags: VALID = the board changed, DONE = is_game_over() of the result. op MOVE_AGENT = the same with
 * BeamSearchAgent._make_move's semantics (agents/beam_search_agent.py:194-258: DOWN returns rot180 of the true result); with
 * *score_inout = 0 before the call the record's score is its merge_score. op SPAWN = Game2048Env.add_new_tile() (:59-67) /
 * BeamSearchAgent._add_random_tile (:260-269): one 2 / 4 on an empty cell by the draw (seed, STEP, index, board_id, counter 1)
 * -- counter 0 is the step's own spawn --, nothing on a full board; flags: VALID = a tile was placed. */
#define G2048_ENV_RECORD_BYTES 80
#define G2048_ENV_OP_STEP  0u
#define G2048_ENV_OP_RESET 1u
#define G2048_ENV_OP_PEEK  2u
#define G2048_ENV_OP_MOVE  3u
#define G2048_ENV_OP_SPAWN 4u
#define G2048_ENV_OP_MOVE_AGENT 5u
#define G2048_ENV_TOKEN_SHIFT 8        /* op | (token << 8), token 0 .. 65535 */
G2048_API int g2048_env_step(void *board_inout, uint32_t *score_inout, uint32_t action, uint32_t op, void *record_out, uint64_t seed,
                   uint64_t index, uint64_t board_id, void *stream);

/* reference state layout (np.int32[16] real tile values, game_2048.py:36,57) <-> packed codes */
G2048_API int g2048_pack_i32(const int32_t *tiles, void *boards_out, size_t n, void *stream);
G2048_API int g2048_unpack_i32(const void *boards, int32_t *tiles_out, size_t n, void *stream);

/* per-shard metrics for the multi-GPU reduction: out[0] = n, out[1] = sum(score), out[2] = #done,
 * out[3] = sum(expanded or 0), out[4..22) = histogram of max code 0..17. out must hold 24 uint64,
 * and is accumulated into (zero it first). flags/expanded may be NULL. */
G2048_API int g2048_metrics(const void *boards, const uint32_t *score, const uint8_t *flags_or_null,
                  const uint32_t *expanded_or_null, unsigned long long *out24, size_t n, void *stream);

/* ---- graph-replayable loops -------------------------------------------------------------------------------
 * The entry points above take the step / decision index as a host scalar, so a captured hipGraph bakes it in. For
 * loops that replay ONE captured move many times (evaluation driver, rollouts), the per-move keys can live in a
 * device key block instead: g2048_keys_advance (one thread) writes the keys of every per-move RNG domain for index
 * *counter into keyblock_out[G2048_KEYBLOCK_WORDS] and increments *counter; the *_dyn variants read their keys (and
 * g2048_track_episodes_dyn its move index) from that block. Results are identical to the scalar forms called with
 * step_index = the counter's value. */
#define G2048_KEYBLOCK_WORDS 16
G2048_API int g2048_keys_advance(uint32_t *keyblock_out, unsigned long long *counter_inout, uint64_t seed, void *stream);
G2048_API int g2048_step_dyn(const void *boards_in, const uint8_t *actions, void *boards_out, uint32_t *score_inout,
                   void *reward_out, uint8_t *flags_out, const uint32_t *keyblock, uint64_t board_id_base, size_t n,
                   uint32_t opts, void *stream);
G2048_API int g2048_beam_get_action_dyn(const void *root_boards, const uint8_t *valid_mask_or_null, uint8_t *action_out,
                              float *prob_out, uint32_t *expanded_out_or_null, int width, int depth,
                              int early_threshold, int mid_threshold, const uint32_t *keyblock,
                              uint64_t game_id_base, size_t n_games, uint32_t opts, void *stream);
G2048_API int g2048_sample_actions_dyn(const float *probs, const uint8_t *mask4_or_null, uint8_t *actions_out, float *prob_out,
                             const uint32_t *keyblock, uint64_t env_id_base, size_t n, void *stream);
G2048_API int g2048_track_episodes_dyn(const uint8_t *flags, const uint32_t *expanded_or_null, uint8_t *alive_inout,
                             int32_t *moves_inout, int32_t *valid_inout, int32_t *invalid_inout,
                             int32_t *milestone_move_inout, unsigned long long *expanded_sum_inout_or_null,
                             const uint32_t *keyblock, size_t n, void *stream);

/* ---- PPO rollout step ---------------------------------------------------------------------------------------
 * One step of a PPO rollout for n envs in ONE launch -- what PPOAgent.get_action's sampling (agents/ppo_agent.py:211-221),
 * Game2048Env.step (environment/game_2048.py:170-210) and the preparation of the next policy call do between two forward
 * passes of the policy: the action is drawn from `probs` (float32 [n][4]) under the valid-move mask exactly as
 * g2048_sample_actions does (draw (seed, POLICY, index, env id)), the env is stepped exactly as g2048_step does (draw
 * (seed, STEP, index, env id); auto-reset in the EPISODE domain), and from the board still in registers the kernel
 * writes the NEXT observation (PPOAgent.normalize_state, :184-195; dtype by the OBS bits of opts) and the NEXT env
 * valid-move mask (game_2048.py:69-95). mask4_in_or_null = NULL: the mask of the current board is computed in place.
 * index = step_index + (step_counter_or_null ? *step_counter_or_null : 0): with a device counter the launch carries no
 * host-side step number, so a hipGraph of a whole T-step rollout (step_index = 0..T-1 baked in, counter += T per replay)
 * can be replayed. Optional outputs for the reward shaping below: next_boards_out (the next state BEFORE any auto-reset)
 * and state_maxcode_out (max log2 code of the state the action was taken in). */
#define G2048_ROLLOUT_OBS_SHIFT 4       /* opts bits 4..5: dtype of obs_next_out */
#define G2048_OBS_F32  0u
#define G2048_OBS_F16  1u
#define G2048_OBS_BF16 2u
G2048_API int g2048_rollout_step(const void *boards_in, const float *probs, const uint8_t *mask4_in_or_null, void *boards_out,
                       uint32_t *score_inout, uint8_t *actions_out, float *prob_out, void *reward_out, uint8_t *flags_out,
                       void *obs_next_out_or_null, uint8_t *mask4_next_out_or_null, void *next_boards_out_or_null,
                       uint8_t *state_maxcode_out_or_null, uint64_t seed, uint64_t step_index,
                       const unsigned long long *step_counter_or_null, uint64_t env_id_base, size_t n, uint32_t opts,
                       void *stream);

/* ---- PPOMemory.sample (agents/ppo_agent.py:21-50) + the head of PPOAgent.update (:342-354) on a device-resident buffer -----
 * `batch` DISTINCT transitions out of n_transitions (np.random.choice(len, batch, replace=False)): sample j is transition P(j),
 * P a bijection of 0 .. n_transitions-1 keyed by (seed, MINIBATCH, sample_index) -- a Feistel network walked until it lands in
 * range --, drawn and gathered by ONE launch with no host round trip. Inputs are the flattened trajectory arrays of a rollout:
 * obs ([n][16] float32 / float16 / bfloat16 per obs_kind = G2048_OBS_*, the normalized states the policy saw), actions (uint8),
 * log_probs (float32), rewards (float32, or float64 when rewards_f64 -- e.g. the shaped reward remember() stores), next_boards
 * (the next states BEFORE any auto-reset, as g2048_rollout_step writes them) and flags. Outputs, what update() turns the sample
 * into: states_out float32 [batch][16], actions_out int64, old_log_probs_out float32, rewards_out float32, next_states_out
 * float32 [batch][16] = normalize_state(next state) (:184-195), dones_out float32 (1.0 = done), and optionally the indices. */
G2048_API int g2048_minibatch_gather(const void *obs, uint32_t obs_kind, const uint8_t *actions, const float *log_probs, const void *rewards,
                           uint32_t rewards_f64, const void *next_boards, const uint8_t *flags, size_t n_transitions, size_t batch,
                           uint64_t seed, uint64_t sample_index, float *states_out, int64_t *actions_out, float *old_log_probs_out,
                           float *rewards_out, float *next_states_out, float *dones_out, int64_t *indices_out_or_null, void *stream);

/* ---- PPOAgent.remember reward shaping (agents/ppo_agent.py:234-269) for an ORDERED batch of n transitions ------------
 * The reference calls remember() once per transition, and two of its terms carry state from call to call: the
 * "new highest tile" bonus (:241-246, self.highest_tile_seen) and the novelty bonus (:259-262, self.seen_states).
 * Batched with exactly the sequential semantics for the order i = 0..n-1 (a rollout buffer [T][N] flattened: step t,
 * then env id), continued across calls through highest_code_inout / the table / index_base:
 *   g2048_shaping_scan    prev_highest_out[i] = max(*highest_code_inout, max log2 code after transitions 0..i-1) -- the
 *                         value highest_tile_seen has when the reference reaches transition i -- and then
 *                         *highest_code_inout = the maximum over everything (device uint32; a fresh agent starts at 1
 *                         = tile 2, ppo_agent.py:171). flags = the flags byte g2048_step / g2048_rollout_step wrote
 *                         (bits 3..7 = max code of the next state). workspace: g2048_shaping_scan_workspace(n) bytes.
 *   g2048_seen_insert     every next state is looked up / inserted in an open-addressing hash set keyed by the whole
 *                         16-byte board (table: 2^capacity_log2 slots of G2048_SEEN_SLOT_BYTES bytes, zero-initialised by
 *                         the caller; keep it at most half full); each key keeps the smallest transition index
 *                         index_base + i that presented it. slot_out[i] = the key's slot. *count_inout grows by the
 *                         number of new keys; *overflow_flag becomes non-zero if the table filled up.
 *   g2048_shaping_apply   shaped_out[i] = the reward remember() stores: env_reward[i] (+ 5.0 * (log2 next_max - log2
 *                         highest so far) if a new highest tile) (+ -2.0 * (log2 current_max - log2 next_max) if the
 *                         max tile fell) + 0.1 * sum(log2 of the 4 largest tiles) (+ 0.2 if transition i is the FIRST
 *                         in order to present its next state) + 0.3 * evaluate_heuristic(next_state), added in that
 *                         order in f64. Call after g2048_seen_insert of the same batch (stream order is enough).
 *   g2048_seen_rehash     re-inserts every key of a table into a larger zeroed one (first indices kept).
 * The only deviation from the reference: its set holds Python hash() values of the board bytes, so two different boards
 * whose 64-bit hashes collide count as one there; here keys are compared in full. */
#define G2048_SEEN_SLOT_BYTES 32
G2048_API size_t g2048_shaping_scan_workspace(size_t n);
G2048_API int g2048_shaping_scan(const uint8_t *flags, uint8_t *prev_highest_out, uint32_t *highest_code_inout, void *workspace,
                       size_t n, void *stream);
G2048_API int g2048_seen_insert(const void *next_boards, uint64_t index_base, void *table, uint32_t capacity_log2,
                      unsigned long long *count_inout, uint32_t *overflow_flag, uint32_t *slot_out, size_t n, void *stream);
G2048_API int g2048_seen_rehash(const void *old_table, uint32_t old_capacity_log2, void *new_table, uint32_t new_capacity_log2,
                      uint32_t *overflow_flag, void *stream);
G2048_API int g2048_shaping_apply(const void *next_boards, const uint8_t *state_maxcode, const uint8_t *flags, const double *env_reward,
                        const uint8_t *prev_highest, const void *table, const uint32_t *slots, uint64_t index_base,
                        double *shaped_out, uint8_t *novel_out_or_null, size_t n, void *stream);


/* PPO actor / critic forward pass of the reference (agents/ppo_agent.py:61-136, ActorNetwork / CriticNetwork in eval mode) on
 * the matrix cores: 16 -> 256 -> 128 -> 64 -> 4 (softmax) for the actor, -> 1 for the critic, with input
 * x = float32(code) / float32(15) read from the packed boards (PPOAgent.normalize_state, as g2048_obs_f32).
 *
 *   g2048_policy_packed_bytes  bytes of one packed network (0 for a bad precision or n_out); a multiple of 16.
 *   g2048_policy_pack          rearranges one network's plain f32 parameters into that blob, on `stream` (no synchronisation;
 *                              packing into the same buffer again updates a forward pass captured in a graph). plain_f32 is
 *                              W1 [256][16], b1 [256], W2 [128][256], b2 [128], W3 [64][128], b3 [64], W4 [n_out][64], b4 [n_out]
 *                              back to back (45,504 + 65 n_out floats, device memory), each weight row-major [out][in] as torch
 *                              stores it. n_out: 4 (actor) or 1 (critic). There is no BatchNorm in the kernel: the caller folds
 *                              every eval-mode BatchNorm1d into a Linear first, with s = gamma / sqrt(running_var + eps) and
 *                              t = beta - running_mean * s:
 *                                BN after a Linear (Linear -> BN -> ReLU):  W' = diag(s) W,  b' = s * b + t;
 *                                BN after a ReLU, i.e. before the next Linear (the reference's relu -> bn -> dropout -> fc):
 *                                                                           W' = W diag(s),  b' = b + W t.
 *                              The reference skips both BatchNorms for a batch of one row (ppo_agent.py:83, :89): such a
 *                              batch takes the parameters without the fold.
 *   g2048_policy_forward       probs_out[i] = softmax(actor(board i)) (float32 n x 4, the input g2048_rollout_step and
 *                              g2048_sample_actions take) and, if critic_packed_or_null is given, value_out_or_null[i] =
 *                              critic(board i), in ONE launch. opts = the precision both blobs were packed with:
 *                                G2048_POLICY_F32   f32 MFMA, exact f32 products and sums (the parity path);
 *                                G2048_POLICY_BF16  weights and the input / hidden activations rounded to bf16 (nearest even),
 *                                                   f32 accumulation, bias and softmax.
 *                              Boards, blobs and probs_out 16-byte aligned, value_out 4-byte aligned. Deterministic: every
 *                              output is one fixed-order accumulation (no split-K, no atomics). Nothing past row n is written. */
#define G2048_POLICY_F32   0
#define G2048_POLICY_BF16  1
G2048_API size_t g2048_policy_packed_bytes(int precision, int n_out);
G2048_API int g2048_policy_pack(const float *plain_f32, int n_out, int precision, void *packed_out, void *stream);
G2048_API int g2048_policy_forward(const void *boards, const void *actor_packed, const void *critic_packed_or_null, float *probs_out,
                         float *value_out_or_null, size_t n, uint32_t opts, void *stream);

/* Forward pass of the reference's transformer policy (models/transformer.py:4-40, TransformerModel in eval mode) on the matrix
 * cores, in ONE launch, read from the packed boards (token t of a board = float32(code of cell t) / float32(15)):
 * Linear(1,64) -> n_layers x nn.TransformerEncoderLayer(d_model 64, 4 heads, dim_ff, ReLU, post-norm, batch_first: x =
 * norm1(x + out_proj(attention(x))), x = norm2(x + linear2(relu(linear1(x)))), scores scaled by 1/4, no mask) -> flatten
 * (token-major, 1024) -> Linear(1024,128) + ReLU -> Linear(128,64) + ReLU -> Linear(64,4) + softmax (probs) and Linear(64,1)
 * (value). d_model, the head count and the 16 tokens are fixed; dim_ff (a multiple of 32) and n_layers (>= 1) are arguments.
 *
 *   g2048_tpolicy_packed_bytes  bytes of the packed blob (0 for a bad argument); a multiple of 16.
 *   g2048_tpolicy_pack          rearranges the plain f32 parameters into that blob, on `stream` (no synchronisation; packing
 *                               into the same buffer again updates a forward pass captured in a graph). plain_f32 holds, back
 *                               to back in the module's state-dict order, every weight row-major [out][in] as torch stores it:
 *                                 embedding.weight [64][1], embedding.bias [64];
 *                                 per layer: in_proj_weight [192][64] (q, k, v rows), in_proj_bias [192], out_proj.weight
 *                                   [64][64], out_proj.bias [64], linear1.weight [dim_ff][64], linear1.bias [dim_ff],
 *                                   linear2.weight [64][dim_ff], linear2.bias [64], norm1.weight [64], norm1.bias [64],
 *                                   norm2.weight [64], norm2.bias [64], then norm1.eps, norm2.eps (two floats, not in the
 *                                   state dict): 16,962 + 129 dim_ff floats;
 *                                 fc1.weight [128][1024], fc1.bias [128], fc2.weight [64][128], fc2.bias [64], actor.weight
 *                                   [4][64], actor.bias [4], critic.weight [1][64], critic.bias [1]: 139,781 floats.
 *   g2048_tpolicy_forward       probs_out[i] (float32 n x 4) and, if value_out_or_null is given, value_out_or_null[i] of
 *                               board i. opts = the precision the blob was packed with:
 *                                 G2048_POLICY_F32   f32 MFMA, exact f32 products and sums (the parity path);
 *                                 G2048_POLICY_BF16  the weights and the matmul inputs of the projections, the feed-forward
 *                                                    and the head layers rounded to bf16 (nearest even), f32 accumulation; the
 *                                                    attention products (Q K^T, P V) stay on the f32 MFMA.
 *                               LayerNorm statistics (biased variance), both softmaxes, the biases and the residual adds are
 *                               f32 in both. Boards, blob and probs_out 16-byte aligned, value_out 4-byte aligned. Every output
 *                               is one fixed-order accumulation (no split-K, no atomics) that does not depend on n or on the
 *                               board's place in the batch. Nothing past row n is written. */
G2048_API size_t g2048_tpolicy_packed_bytes(int precision, int dim_ff, int n_layers);
G2048_API int g2048_tpolicy_pack(const float *plain_f32, int dim_ff, int n_layers, int precision, void *packed_out, void *stream);
G2048_API int g2048_tpolicy_forward(const void *boards, const void *packed, float *probs_out, float *value_out_or_null, size_t n,
                          int dim_ff, int n_layers, uint32_t opts, void *stream);

/* Complete games of the PPO actor (play.py:44-68, train.py:54-90), every game played to the end on the device in ONE launch,
 * as g2048_play_games does for the beam agent. Game g (global id game_id_base + g) starts from boards_inout[g] /
 * score_inout[g]; at move t = 0, 1, ... it takes p = softmax(actor(board)) -- bit for bit what g2048_policy_forward gives for
 * the same board and blob (actor_packed, packed with the precision in opts) -- then the action by mode:
 *   MASKED    train.py:56-61, agent.get_action(state, env.get_valid_moves()): exactly g2048_sample_actions(step_index = t,
 *             env id = game id) with the env's valid-move mask (draw (seed, POLICY, t, game id));
 *   UNMASKED  play.py:46, agent.get_action(state): the same with all four actions allowed. Like g2048_sample_actions with no
 *             mask it samples from p_a + 1e-10, which differs from Categorical(probs) by at most 4e-10 in probability;
 *   GREEDY    not in the reference: the argmax of p over the valid moves, ties to the lowest index (torch.argmax); no draw;
 * and steps the board exactly as g2048_step(step_index = t, board id = game id) does, without auto-reset. The game ends when
 * it is over (DONE) or after max_moves moves. Outputs per game: final board and score (in place), moves, valid / invalid
 * move counts, milestone_move_out[g][0..8) = the move at which tiles 64..8192 first appeared (-1 = never; as
 * g2048_track_episodes records them), alive_out[g] = 1 if the game hit max_moves without finishing, reward_sum_out_or_null[g]
 * = the f64 env rewards (game_2048.py:212-277) summed in move order from 0.0 (train.py's episode_reward, play.py's
 * total_reward), and actions_out_or_null = the move-set, max_moves bytes per game, 0xFF from the game's end on (the layout of
 * g2048_play_games: g2048_replay_games rebuilds every intermediate board; the library fills it with 0xFF first).
 * opts = precision (G2048_POLICY_*) | mode << G2048_PLAY_POLICY_MODE_SHIFT. max_waves = the number of wavefronts (32 games in
 * flight per wavefront in f32, 64 in bf16; a finished game's slot takes the next game), 0 = as many as the chip holds at once;
 * the games do not depend on it. workspace: g2048_play_policy_workspace(n_games) bytes of device memory, 8-byte aligned (a
 * ticket counter the call clears on `stream`). Boards, weights and milestone_move_out 16-byte aligned, rewards 8, the rest 4.
 * Nothing past game n_games is written. */
#define G2048_PLAY_POLICY_MASKED   0u   /* train.py:56-61 */
#define G2048_PLAY_POLICY_UNMASKED 1u   /* play.py:46 */
#define G2048_PLAY_POLICY_GREEDY   2u   /* argmax over the valid moves (not in the reference) */
#define G2048_PLAY_POLICY_MODE_SHIFT 4
G2048_API size_t g2048_play_policy_workspace(size_t n_games);
G2048_API int g2048_play_policy_games(void *boards_inout, uint32_t *score_inout, const void *actor_packed, int32_t *moves_out,
                            int32_t *valid_out, int32_t *invalid_out, int32_t *milestone_move_out, double *reward_sum_out_or_null,
                            uint8_t *alive_out, uint8_t *actions_out_or_null, int max_moves, uint64_t seed, uint64_t game_id_base,
                            size_t n_games, uint32_t opts, uint32_t max_waves, void *workspace, size_t workspace_bytes, void *stream);

/* Complete games of the transformer policy (the network of g2048_tpolicy_forward), every game played to the end on the device
 * in ONE launch, as g2048_play_policy_games does for the PPO actor: the same games, modes, draws and outputs, with the
 * transformer's probabilities. Game g (global id game_id_base + g) starts from boards_inout[g] / score_inout[g]; at move t = 0,
 * 1, ... it takes p = the probs g2048_tpolicy_forward gives for the same board and blob (packed with the precision in opts;
 * dim_ff, n_layers as packed), bit for bit, then the action by mode:
 *   MASKED    exactly g2048_sample_actions(step_index = t, env id = game id) with the env's valid-move mask (draw (seed, POLICY,
 *             t, game id));
 *   UNMASKED  the same with all four actions allowed (it samples from p_a + 1e-10, as g2048_sample_actions with no mask);
 *   GREEDY    the argmax of p over the valid moves, ties to the lowest index (torch.argmax); no draw;
 * and steps the board exactly as g2048_step(step_index = t, board id = game id) does, without auto-reset. The game ends when it
 * is over (DONE) or after max_moves moves. Outputs per game: final board and score (in place), moves, valid / invalid move
 * counts, milestone_move_out[g][0..8) = the move at which tiles 64..8192 first appeared (-1 = never; as g2048_track_episodes
 * records them), alive_out[g] = 1 if the game hit max_moves without finishing, reward_sum_out_or_null[g] = the f64 env rewards
 * summed in move order from 0.0, and actions_out_or_null = the move-set, max_moves bytes per game, 0xFF from the game's end on
 * (the input of g2048_replay_games; the library fills it with 0xFF first).
 * opts = precision (G2048_POLICY_*) | mode (G2048_PLAY_POLICY_*) << G2048_PLAY_POLICY_MODE_SHIFT. max_blocks = the number of
 * blocks (16 games in flight per block of four wavefronts; a finished game's slot takes the next game), 0 = as many as the chip
 * holds at once; the games do not depend on it. workspace: g2048_play_tpolicy_workspace(n_games) bytes of device memory, 8-byte
 * aligned (a ticket counter the call clears on `stream`). Boards, blob and milestone_move_out 16-byte aligned, rewards 8, the
 * rest 4. Arguments are checked before any device call; n_games == 0 returns G2048_OK. Nothing past game n_games is written. */
G2048_API size_t g2048_play_tpolicy_workspace(size_t n_games);
G2048_API int g2048_play_tpolicy_games(void *boards_inout, uint32_t *score_inout, const void *packed, int dim_ff, int n_layers,
                             int32_t *moves_out, int32_t *valid_out, int32_t *invalid_out, int32_t *milestone_move_out,
                             double *reward_sum_out_or_null, uint8_t *alive_out, uint8_t *actions_out_or_null, int max_moves,
                             uint64_t seed, uint64_t game_id_base, size_t n_games, uint32_t opts, uint32_t max_blocks, void *workspace,
                             size_t workspace_bytes, void *stream);

/* Forward pass of the hybrid agent's CNN-transformer Q-network (agents/hybrid.py:700-727, HybridDQN) on the matrix cores, in ONE
 * launch, read from the packed boards. Per board, with x = the 16 raw tile values as float32 (2 ** code, 0 for empty: the env's
 * get_state(), not the / 15 of the policies): Conv2d(1,32,k=2,s=1,p=1) + ReLU (32 x 5 x 5) -> Conv2d(32,64,k=2,s=1,p=0) + ReLU
 * (64 x 4 x 4) -> flatten channel-major (feature c * 16 + y * 4 + x) -> Linear(1024,128) -> n_layers x
 * nn.TransformerEncoderLayer(d_model 128, dim_ff, ReLU, post-norm) -> Linear(128,4) = Q[4].
 *   Sequence length 1. The reference builds the layer without batch_first and feeds it x.unsqueeze(1), so a batch of B boards is ONE
 *     sequence of B tokens that attend to each other; it only ever calls the network with one board. Every board here is its own
 *     sequence of one token: row i is model(x[i:i+1]), equally the module with the encoder input reshaped to (1, B, 128). The
 *     softmax over one key is exactly 1.0, so the attention block is out_proj(W_v x + b_v): a layer is x = norm1(x +
 *     out_proj(v(x))), x = norm2(x + linear2(relu(linear1(x)))). Q, K and the head count cannot influence the result and are
 *     not read.
 *   Eval mode. The reference never calls .eval(), so its dropout is live even in select_action; this is the eval-mode function,
 *     as the two policies are.
 * The widths 32, 64, 1024 and 128 are fixed; dim_ff (a multiple of 32) and n_layers (>= 1) are arguments.
 *
 *   g2048_qnet_packed_bytes  bytes of the packed blob (0 for a bad argument); a multiple of 16.
 *   g2048_qnet_pack          rearranges the plain f32 parameters into that blob, on `stream` (no synchronisation; packing into
 *                            the same buffer again updates later forward passes). plain_f32 holds, back to back in the module's
 *                            state-dict order, every weight row-major [out][in] as torch stores it:
 *                              cnn.0.weight [32][1][2][2], cnn.0.bias [32], cnn.2.weight [64][32][2][2], cnn.2.bias [64],
 *                                embedding.weight [128][1024], embedding.bias [128]: 139,616 floats;
 *                              per layer: in_proj_weight [384][128] and in_proj_bias [384] whole (only the V rows 256..383 are
 *                                used), out_proj.weight [128][128], out_proj.bias [128], linear1.weight [dim_ff][128],
 *                                linear1.bias [dim_ff], linear2.weight [128][dim_ff], linear2.bias [128], norm1.weight [128],
 *                                norm1.bias [128], norm2.weight [128], norm2.bias [128], then norm1.eps, norm2.eps (two floats,
 *                                not in the state dict): 66,690 + 257 dim_ff floats;
 *                              fc.weight [4][128], fc.bias [4]: 516 floats.
 *                            In all 140,132 + n_layers (66,690 + 257 dim_ff) floats (the reference's dim_ff 2048, 2 layers:
 *                            1,326,180 parameters + 4 eps).
 *   g2048_qnet_forward       q_out[i] (float32 n x 4) = Q of board i and, if actions_out_or_null is given, actions_out_or_null[i]
 *                            = the exploit action of DQNAgent.select_action (hybrid.py:943-953): Q of every move that is invalid
 *                            under the env's valid-move mask of that board (G2048_VALID_ENV semantics) replaced by -1e9, then the
 *                            argmax with ties to the lowest index (np.argmax); a board with no valid move gets action 0. q_out
 *                            holds the Q-values as computed, without that replacement. opts = the precision the blob was packed
 *                            with:
 *                              G2048_POLICY_F32   f32 MFMA, exact f32 products and sums (the parity path);
 *                              G2048_POLICY_BF16  the weights and the matmul inputs of conv2 and of every Linear rounded to bf16
 *                                                 (nearest even), f32 accumulation; conv1 stays in f32.
 *                            LayerNorm statistics (biased variance), the biases and the residual adds are f32 in both. Boards,
 *                            blob and q_out 16-byte aligned. Every output is one fixed-order accumulation (no split-K, no
 *                            atomics) that does not depend on n, on the board's place in the batch or on the launch geometry.
 *                            Arguments are checked before any device call; n == 0 returns G2048_OK. Nothing past row n is
 *                            written. */
G2048_API size_t g2048_qnet_packed_bytes(int precision, int dim_ff, int n_layers);
G2048_API int g2048_qnet_pack(const float *plain_f32, int dim_ff, int n_layers, int precision, void *packed_out, void *stream);
G2048_API int g2048_qnet_forward(const void *boards, const void *packed, float *q_out, uint8_t *actions_out_or_null, size_t n, int dim_ff,
                       int n_layers, uint32_t opts, void *stream);

/* DQNAgent.select_action (agents/hybrid.py:909-953) for n boards in ONE launch, given their Q-values: the epsilon-greedy choice
 * between the exploit action of g2048_qnet_forward and the reference's biased exploration. Board i has id env_id_base + i; with
 * (k0, k1) = the keys of (seed, POLICY domain, step_index):
 *   coin     u = (float)(draw(k0, k1, id, 1) >> 8) * 2^-24; the board explores iff u < epsilon, compared in f32 (hybrid.py:912).
 *            epsilon 0 never explores, epsilon 1 always does.
 *   exploit  (:943-953) exactly the rule of g2048_qnet_forward's actions: Q of every move that is invalid under the env's mask
 *            replaced by -1e9, the argmax with ties to the lowest index, action 0 for a board with no valid move.
 *   explore  (:914-936) random.choices(valid_actions, weights): the preferences over the actions 0..3 are (1, 1, 3, 3) (RIGHT and DOWN
 *            three times as likely) when the board's max tile is >= 64 and np.argmax(board) is cell (3,3), i.e. cell 15's code is >= 6 and
 *            strictly greater than every other cell's, and (1, 1, 1, 1) otherwise; the action is what g2048_sample_actions draws
 *            from p = (0.125, 0.125, 0.375, 0.375) or (0.25, 0.25, 0.25, 0.25) under the env's valid-move mask with draw(k0, k1,
 *            id, 0). Those p are exact in f32 and the sampler's + 1e-10 does not change them. A board with no valid move samples
 *            among all four (the reference's random.randint(0, 3), :918-919).
 *   The reference's beam_search branch of select_action (:814-907) is not part of this launch, which is select_action with
 *   use_beam_search = False; g2048_qnet_beam_actions is the one with it.
 * q: float32 (n,4), 16-byte aligned, as g2048_qnet_forward wrote it; boards 16-byte aligned; explored_out_or_null[i] = 1 where
 * the board explored. epsilon outside [0, 1] or NaN is refused. Arguments are checked before any device call; n == 0 returns
 * G2048_OK. Nothing past row n is written. */
G2048_API int g2048_qnet_select_actions(const float *q, const void *boards, uint8_t *actions_out, uint8_t *explored_out_or_null,
                              float epsilon, uint64_t seed, uint64_t step_index, uint64_t env_id_base, size_t n, void *stream);

/* Complete games of the Q-network (the reference's evaluate_agent, hybrid.py:1176-1210: select_action -> env.step until done),
 * every game played to the end on the device in ONE launch, as g2048_play_tpolicy_games does for the transformer policy: the same
 * games, draws and outputs. Game g (global id game_id_base + g) starts from boards_inout[g] / score_inout[g]; at move t = 0, 1,
 * ... it takes Q = what g2048_qnet_forward gives for the same board and blob (packed with the precision in opts; dim_ff, n_layers
 * as packed), bit for bit, then the action exactly as g2048_qnet_select_actions(epsilon, step_index = t, id = game id) picks it
 * (epsilon 0: the exploit action, no draw; use_beam_search = False, as there), and steps the board exactly as
 * g2048_step(step_index = t, board id = game id) does, without auto-reset. The game ends when it is over (DONE) or after
 * max_moves moves. Outputs per game: final board and score (in place), moves, valid / invalid move counts,
 * milestone_move_out[g][0..8) = the move at which tiles 64..8192 first appeared (-1 = never), alive_out[g] = 1 if the game hit
 * max_moves without finishing, reward_sum_out_or_null[g] = the f64 env rewards summed in move order from 0.0, and
 * actions_out_or_null = the move-set, max_moves bytes per game, 0xFF from the game's end on (the input of g2048_replay_games; the
 * library fills it with 0xFF first).
 * opts = the precision alone (G2048_POLICY_*). max_waves = the number of wavefronts, each of which holds 32 game slots and runs
 * the network on them by itself (a finished game's slot takes the next game), 0 = as many as the chip holds at once; the games do
 * not depend on it. workspace: g2048_play_qnet_workspace(n_games) bytes of device memory, 8-byte aligned (a ticket counter the
 * call clears on `stream`). Boards, blob and milestone_move_out 16-byte aligned, rewards 8, the rest 4. Arguments are checked
 * before any device call; n_games == 0 returns G2048_OK. Nothing past game n_games is written. */
G2048_API size_t g2048_play_qnet_workspace(size_t n_games);
G2048_API int g2048_play_qnet_games(void *boards_inout, uint32_t *score_inout, const void *packed, int dim_ff, int n_layers,
                          int32_t *moves_out, int32_t *valid_out, int32_t *invalid_out, int32_t *milestone_move_out,
                          double *reward_sum_out_or_null, uint8_t *alive_out, uint8_t *actions_out_or_null, int max_moves,
                          float epsilon, uint64_t seed, uint64_t game_id_base, size_t n_games, uint32_t opts, uint32_t max_waves,
                          void *workspace, size_t workspace_bytes, void *stream);

/* DQNAgent.select_action with use_beam_search = True (agents/hybrid.py:909-953, the reference's own setting: beam_width 15,
 * search_depth 30, beam_search_threshold 64, gamma 0.99), and the games played that way.
 *
 * What the reference's beam_search (:814-907) computes. Its loop over the depth ends after the first level whatever search_depth
 * is: the early-exit test (:871) reads the fourth field of a beam entry as `done`, and that field is the transition probability,
 * which is never 0. So a decision is one ranking of the root's children, and at search_depth >= 2 -- the reference's 30 included --
 * the network is never consulted on a planned board (leaf values are taken only at the last step) and the random draws cannot
 * change the result (the reward of a candidate depends on the moved board and the spawned tile's value, not on its cell). With the
 * reference's settings the network therefore decides only boards whose max tile is below 64 or that hold fewer than 8 tiles.
 *   planned     the search decides board B when its max tile >= threshold and at least 8 cells are filled; otherwise the exploit
 *               action of g2048_qnet_forward does, as in g2048_qnet_select_actions.
 *   candidates  in the order a = 0, 1, 2, 3 (LEFT, UP, RIGHT, DOWN, all four directions true as in the env). M = move(B, a). M == B:
 *               one candidate, reward -1.0, p = 1.0. Else, e = empty cells of M, k = min(3, e): 2k candidates -- pick 0 with a 2,
 *               pick 0 with a 4, pick 1 with a 2, ... -- with the rewards of g2048_simulate_move_sampled (weighted 0.9 / 0.1) and
 *               p = 1.0 / (2k). Slot 8 a + j is candidate j of action a.
 *   totals      search_depth >= 2: 0.0 + reward. search_depth == 1: (0.0 + reward) + gamma * (double)v, v = the float32 maximum of
 *               the four Q-values of the candidate's board (an invalid move's board is B itself). Finite values are assumed.
 *   beam        key = total * p in f64; the first beam_width candidates in descending key order, equal keys in candidate order.
 *   action      the beam is walked in order, every action sums the keys of its members in that order; the largest sum wins, equal
 *               sums go to the action whose first member stands earliest in the beam.
 * All of it is f64 in the reference's operation order and bit-exact (tests/golden/qnet_beam.npz).
 *
 *   g2048_qnet_beam_actions   g2048_qnet_select_actions with that exploit action, one launch: the same coin, the same
 *                             exploration, the same draws. planned_out_or_null[i] = 1 where board i is planned (whether or not it
 *                             then explored). succ_q_or_null: float32 (n, 32, 4), 16-byte aligned, Q of slot 8 a + j as
 *                             g2048_qnet_forward wrote it for the boards of g2048_qnet_beam_expand; required at search_depth 1 and
 *                             not read otherwise. beam_width 1 .. 64, search_depth >= 1, threshold (a tile value) >= 1, gamma finite.
 *   g2048_qnet_beam_expand    the candidate boards for search_depth 1: succ_boards_out (n x 32 boards, 16-byte aligned), slot 8 a + j;
 *                             count_out (uint8 n x 4, 4-byte aligned) = candidates per action. Pick i of action a of board
 *                             state_id_base + b uses draw 3 a + i of (seed, SIMULATE domain, step_index, that id) with
 *                             g2048_simulate_move_sampled's mapping (for a = 0 its very successors). An invalid move has count 1 and
 *                             the board itself in slot 8 a; unused slots hold the empty board.
 *   g2048_play_qnet_beam_games / _workspace   g2048_play_qnet_games with beam_width, search_depth and threshold after epsilon:
 *                             the same launch, games, draws and outputs, the exploit action of a planned board being the search's.
 *                             search_depth >= 2 only: search_depth 1 needs the network per candidate and is refused (play it
 *                             move by move with the three launches above).
 * Arguments are checked before any device call; n == 0 returns G2048_OK before any check. Nothing past row n is written. */
G2048_API int g2048_qnet_beam_actions(const float *q, const void *boards, const float *succ_q_or_null, uint8_t *actions_out,
                            uint8_t *planned_out_or_null, uint8_t *explored_out_or_null, int beam_width, int search_depth,
                            int threshold, double gamma, float epsilon, uint64_t seed, uint64_t step_index, uint64_t env_id_base,
                            size_t n, void *stream);
G2048_API int g2048_qnet_beam_expand(const void *boards, void *succ_boards_out, uint8_t *count_out, uint64_t seed, uint64_t step_index,
                           uint64_t state_id_base, size_t n, void *stream);
G2048_API size_t g2048_play_qnet_beam_workspace(size_t n_games);
G2048_API int g2048_play_qnet_beam_games(void *boards_inout, uint32_t *score_inout, const void *packed, int dim_ff, int n_layers,
                               int32_t *moves_out, int32_t *valid_out, int32_t *invalid_out, int32_t *milestone_move_out,
                               double *reward_sum_out_or_null, uint8_t *alive_out, uint8_t *actions_out_or_null, int max_moves,
                               float epsilon, int beam_width, int search_depth, int threshold, uint64_t seed, uint64_t game_id_base,
                               size_t n_games, uint32_t opts, uint32_t max_waves, void *workspace, size_t workspace_bytes, void *stream);
/* ---- the hybrid agent's prioritized experience replay ("per") and train_step's reward shaping, on the device --------------
 * PrioritizedReplayBuffer (agents/hybrid.py:730-765) and the part of DQNAgent.train_step around it that needs no gradient
 * (:959-969 the batch as tensors, :971-1034 the shaping, :1063-1064 the new priorities). The gradient step stays the caller's.
 *
 * The buffer is a ring of `capacity` slots in caller-owned device arrays: states and next_states (packed boards, 16 bytes
 * each, 16-byte aligned), actions (uint8), rewards (float32), dones (uint8), priorities (float32). The caller tracks `size`
 * (live entries, <= capacity) and `head` (the physical slot of the oldest entry, < capacity) and passes both by value.
 * Logical index i (0 = oldest: the reference's deque index) lives at slot (head + i) % capacity; every index that crosses this
 * interface is logical. Nothing here synchronises; every call is a few launches on `stream`.
 *
 *   g2048_per_push   m calls of push (:736-740) in order: boards / next_boards (the next states BEFORE any auto-reset, as
 *       g2048_step and g2048_rollout_step write them), actions_in, rewards_in (float32, or float64 when rewards_f64: rounded to
 *       float32 as torch.tensor(rewards, dtype=float32) does, :966) and flags (bit 0 = done). Every new entry gets the priority
 *       M = the maximum of the `size` live priorities before the call, 1.0 for an empty buffer. That is exact: the first push
 *       appends M itself, so no eviction during the batch can lower the maximum. Entry k goes to slot (head + size + k) %
 *       capacity; afterwards the caller's size is min(size + m, capacity) and its head has advanced by the entries evicted,
 *       max(0, size + m - capacity). m > capacity is refused. workspace: g2048_per_update_workspace(capacity) bytes.
 *   g2048_per_sample   sample (:742-757) and the head of train_step, `batch` draws with replacement:
 *         w_i = priorities_i ^ alpha and probs_i = w_i / sum(w) in float32 (the sum is accumulated in float64 in a fixed order);
 *         cdf = the running sum of (double)probs in logical order, divided by its last entry (np.random.choice);
 *         indices_out[j] = the number of cdf entries <= u_j (searchsorted(side='right'); a draw >= 1 gives the last entry);
 *         weights_out[j] = (size * probs[index_j]) ^ (-beta) in float32, divided by the batch's maximum (:754-755);
 *         states_out / next_states_out float32 [batch][16] (the tile values 2^code, 0 = empty), actions_out int64, rewards_out,
 *         dones_out float32 (:964-968); shaped_out = g2048_dqn_shape_rewards of the gathered transitions; probs_out_or_null
 *         float32 [size].
 *       u_j = u_or_null[j] (float64, device memory) when given, else h_j * 2^-32 with h_j draw 0 of (seed, REPLAY domain,
 *       sample_index, id j). size < batch is refused: train_step returns before it samples then (:956-957). The scan is made
 *       of stream-ordered launches over tiles of G2048_PER_SCAN_TILE entries (tile sums, one wave over the sums, the final
 *       pass); no block waits for another and no floating-point sum goes through an atomic, so two calls give the same bits.
 *       workspace: g2048_per_sample_workspace(size, batch) bytes, 16-byte aligned. The buffer is not modified.
 *   g2048_dqn_shape_rewards   the shaping loop (:971-1034) for any n (state, next state, reward) triples, bit for bit: the
 *       mixed float32 / float64 arithmetic of the reference's NumPy scalars is kept (csrc/g2048_per.h states each step).
 *   g2048_per_update_priorities   update_priorities(indices, td_errors + 1e-5) (:1063-1064, :759-762): entry indices[j] gets
 *       max(float32(td_errors[j] + 1e-5f), 1e-5f); indices outside 0 .. size-1 are ignored; of duplicate indices the occurrence
 *       latest in the batch wins, as in the reference's loop (decided by an integer maximum of the batch position, not by write
 *       order). workspace: g2048_per_update_workspace(capacity) bytes, contents irrelevant.
 * Arguments are checked before any device call. */
#define G2048_PER_SCAN_TILE 256
G2048_API size_t g2048_per_update_workspace(size_t capacity);
G2048_API int g2048_per_push(void *states, void *next_states, uint8_t *actions, float *rewards, uint8_t *dones, float *priorities,
                   size_t capacity, size_t size, size_t head, const void *boards, const void *next_boards,
                   const uint8_t *actions_in, const void *rewards_in, uint32_t rewards_f64, const uint8_t *flags, size_t m,
                   void *workspace, void *stream);
G2048_API size_t g2048_per_sample_workspace(size_t size, size_t batch);
G2048_API int g2048_per_sample(const void *states, const void *next_states, const uint8_t *actions, const float *rewards,
                     const uint8_t *dones, const float *priorities, size_t capacity, size_t size, size_t head, float alpha,
                     float beta, size_t batch, uint64_t seed, uint64_t sample_index, const double *u_or_null, void *workspace,
                     int64_t *indices_out, float *weights_out, float *states_out, int64_t *actions_out, float *rewards_out,
                     float *next_states_out, float *dones_out, float *shaped_out, float *probs_out_or_null, void *stream);
G2048_API int g2048_dqn_shape_rewards(const void *states, const void *next_states, const float *rewards, size_t n, float *shaped_out,
                            void *stream);
G2048_API int g2048_per_update_priorities(float *priorities, size_t capacity, size_t size, size_t head, const int64_t *indices,
                                const float *td_errors, size_t batch, void *workspace, void *stream);

/* ---- the Q-network's BATCH forward and train_step's Double-DQN targets (agents/hybrid.py:1038-1046) ----------------------
 * train_step calls the module of g2048_qnet_forward on a whole batch. Its encoder layer is not batch_first and is fed
 * x.unsqueeze(1), so the n boards are ONE sequence of n tokens that attend to each other: per layer the whole in_proj (Q, K, V),
 * 8 heads of dimension 16, scores q.k / 4 over all n keys, softmax (f32, the row maximum subtracted), P.V, out_proj, residual,
 * norm1, the feed-forward pair, norm2; then fc. Row i of the result depends on every board of the call; n = 1 is
 * g2048_qnet_forward's function. Eval mode (no dropout), 8 heads only.
 *
 *   g2048_qnet_forward_batch   q_out (float32 n x 4) = the module's eval-mode output on the n boards as one call. WEIGHTS: the
 *       PLAIN f32 buffer that g2048_qnet_pack takes as its input (layout above, 16-byte aligned), read directly: there is no
 *       second packed blob, and whoever keeps that buffer current keeps this entry point current. f32 only (f32 MFMA, f32
 *       softmax): the embedding is unnormalised and the inputs are tile values up to 131,072, the first layer's logits reach
 *       1e9 and its softmax is nearly one-hot; bf16 logits would pick keys at random. The call is 2 + 5 n_layers launches on
 *       `stream` (conv; embedding; per layer in_proj, attention, out_proj + norm1, linear1, linear2 + norm2, the last with fc),
 *       the activations between them in `workspace`: g2048_qnet_batch_workspace(n, dim_ff) bytes of device memory, 16-byte
 *       aligned, contents irrelevant before and meaningless after. Every output element is one wavefront's fixed-order
 *       accumulation (no split-K, no atomics): two calls give the same bits. The order of the boards matters to the last bits
 *       (the keys are summed in call order). 1 <= n <= G2048_QNET_BATCH_MAX; a larger n is refused, not truncated; n == 0
 *       returns G2048_OK and does nothing. Nothing past row n of q_out is written.
 *   g2048_qnet_batch_workspace   that size; 0 for n == 0, n > G2048_QNET_BATCH_MAX or a bad dim_ff. Non-decreasing in n.
 *   g2048_dqn_targets   hybrid.py:1042-1046 in one launch, given q_online_next and q_target_next (float32 n x 4, 16-byte aligned: two
 *       g2048_qnet_forward_batch calls on the next states), shaped and dones (float32 [n], as g2048_per_sample writes them):
 *         next_actions_out[i] (int64) = argmax of q_online_next[i], UNMASKED (the reference applies no valid-move mask here), the
 *           first maximum on ties;
 *         targets_out[i] (float32) = shaped[i] + ((1 - dones[i]) * gamma) * q_target_next[i][next_actions_out[i]], each of the
 *           three operations rounded to float32, no fused multiply-add: torch's `shaped + (1 - dones) * gamma * next_q` on the
 *           same Q, bit for bit.
 * Arguments are checked before any device call (null, misaligned, dim_ff not a multiple of 32, n_layers < 1, n too large). */
#define G2048_QNET_BATCH_MAX 4096
G2048_API size_t g2048_qnet_batch_workspace(size_t n, int dim_ff);
G2048_API int g2048_qnet_forward_batch(const void *boards, const float *plain_f32, float *q_out, size_t n, int dim_ff, int n_layers,
                             void *workspace, void *stream);
G2048_API int g2048_dqn_targets(const float *q_online_next, const float *q_target_next, const float *shaped, const float *dones,
                      float gamma, int64_t *next_actions_out, float *targets_out, size_t n, void *stream);

/* ---- the Q-network's loss and gradient pass (agents/hybrid.py:1038, :1049-1055) ------------------------------------------
 * The lines of train_step that need gradients, for the module of g2048_qnet_forward_batch (eval mode, f32, 8 heads, the n boards
 * ONE sequence). The reference runs them with its dropout live. These entry points are the eval-mode function; the same passes
 * with the dropout are the training entry points of the second library (include/g2048_train.h: g2048_qnet_forward_batch_dropout,
 * g2048_qnet_loss_grad_dropout), whose p = 0 is this function bit for bit. Acting (g2048_qnet_forward, g2048_qnet_select_actions, the
 * play entry points) has no dropout in either library.
 *
 *   g2048_qnet_loss_grad   given boards (uint8 n x 16), actions (int64 [n]), targets and weights (float32 [n]):
 *         q_out (float32 n x 4)  = the bits of g2048_qnet_forward_batch on the same boards and weights;
 *         d = q_out[i][actions[i]] - targets[i];
 *         td_out[i] = 0.5 d^2 if |d| < 1 else |d| - 0.5       (nn.SmoothL1Loss(reduction='none'), beta 1);
 *         loss_out[0] = mean(weights[i] * td_out[i]);
 *         grad_out = d loss / d parameter for every parameter, g2048_qnet_plain_floats(dim_ff, n_layers) floats laid out exactly
 *           like the plain buffer (so that parameter t's gradient is the slice at t's offset); the two LayerNorm-eps slots of
 *           every layer are written as 0. grad_out is OVERWRITTEN, never accumulated into.
 *       An action outside 0 .. 3 is the caller's error: the kernel uses actions[i] & 3, so nothing is read out of bounds.
 *       The forward keeps its activations in `workspace` (g2048_qnet_grad_workspace(n, dim_ff, n_layers) bytes of device memory,
 *       16-byte aligned, contents irrelevant before and meaningless after); the backward is one phase per launch on `stream`:
 *       the head, LayerNorm backward, data-gradient and weight-gradient products on the f32 matrix cores, the attention backward
 *       in two kernels (the probabilities recomputed from qkv and the forward's row maximum and sum), the convolutions' on the
 *       VALU. No atomics, no split-K across blocks: every gradient element is one fixed-order accumulation, sums over the boards
 *       per tile of 16 and then over the tiles in order, so two calls give the same bits. Nothing past row n of q_out and
 *       td_out or past the stated sizes is written. 1 <= n <= G2048_QNET_BATCH_MAX (a larger n is refused, not truncated); n == 0
 *       returns G2048_OK and does nothing. f32 only, for the reason g2048_qnet_forward_batch gives.
 *       The first layer's softmax is nearly one-hot on raw tile values (logits up to 1e9): at n >= 2 on boards with large tiles
 *       the gradients that pass through it (the convolutions', the embedding's, layer 0's in_proj) are not a float32 quantity in
 *       ANY float32 implementation, stock torch included; they are computed all the same.
 *   g2048_qnet_grad_workspace   that size; 0 for n == 0, n > G2048_QNET_BATCH_MAX, a bad dim_ff or n_layers. Non-decreasing in n.
 * Arguments are checked before any device call (null, misaligned, dim_ff not a multiple of 32, n_layers < 1, n too large). */
G2048_API size_t g2048_qnet_grad_workspace(size_t n, int dim_ff, int n_layers);
G2048_API int g2048_qnet_loss_grad(const void *boards, const float *plain_f32, const int64_t *actions, const float *targets,
                         const float *weights, size_t n, int dim_ff, int n_layers, float *grad_out, float *td_out, float *loss_out,
                         float *q_out, void *workspace, void *stream);
/* ---- the Q-network's gradient clipping and AdamW update (agents/hybrid.py:1057-1058) ---------------------------------------
 * clip_grad_norm_(parameters, max_norm) and AdamW.step() of train_step over the whole network at once: the parameters are the
 * PLAIN f32 buffer (layout above), the gradients the buffer g2048_qnet_loss_grad fills, the two moment estimates two more
 * buffers of the same layout that start as zeros. All four hold 140132 + n_layers * (66690 + 257 * dim_ff) floats and are
 * 16-byte aligned.
 *
 *   g2048_qnet_adamw_step   update number `step` (>= 1), two launches on `stream`, no host synchronisation:
 *       1. the gradient norm. Block b adds grad[i]^2 over chunk b of the buffer in a fixed order and writes one partial sum to
 *          `workspace`. The chunks are equal, a multiple of 1,024 floats and a function of the float count ALONE (never of the
 *          device's compute units); there are at most G2048_QNET_STEP_MAX_PARTIALS of them for every accepted dim_ff and
 *          n_layers. Squares, partial sums and the total are f64, so the norm is the f64 norm to f32 rounding.
 *       2. clip and update. Every block adds all partials up again in the same order, so all hold the same norm;
 *          norm_out[0] = (float)sqrt(total). If that is not finite (an inf or a NaN in grad) the launch writes NOTHING else:
 *          plain, grad, exp_avg and exp_avg_sq keep their bits (stock torch would write NaN into every weight). Otherwise, with
 *          c = min(1, max_norm / (norm + 1e-6)) (clip_grad_norm_'s rule, evaluated as torch evaluates it in f32: the reciprocal of
 *          norm + 1e-6, times max_norm; max_norm = +inf: no clipping), for every element:
 *              g = grad[i] * c;  grad[i] = g                      (grad is left clipped, as clip_grad_norm_ leaves it)
 *              p = plain[i] * (1 - lr * weight_decay)
 *              m = m + (g - m) * (1 - beta1)
 *              v = v * beta2 + (g * g) * (1 - beta2)
 *              p = p - (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps))     bc1 = 1 - beta1^step, bc2 = 1 - beta2^step
 *          every operation rounded to f32 on its own, in the order of torch's AdamW. 1 - lr * weight_decay, 1 - beta1, 1 - beta2,
 *          lr / bc1 and sqrt(bc2) are formed on the host in f64 and passed to the kernel as floats, as torch forms them from its
 *          Python scalars; for that beta1 and beta2 are read as the shortest decimal that rounds to the float given (0.999f
 *          is 0.999: 1 - (double)0.999f would be 1.3e-5 off 0.001).
 *          The two LayerNorm-eps slots of every layer (the last two floats of each layer's block) are settings, not parameters:
 *          all four buffers keep their bits there (grad, exp_avg and exp_avg_sq are 0 there and stay 0; weight decay would
 *          otherwise shrink the eps by lr * weight_decay a step). grad there is part of the norm like any other element.
 *       No atomics, no block waits on another: two calls from the same state give the same bits. Nothing outside the four
 *       buffers, norm_out[0] and the workspace is written.
 *   g2048_qnet_step_workspace   bytes of `workspace` (device memory, 16-byte aligned, contents irrelevant before and meaningless
 *       after): one f64 per partial sum, at most 8 * G2048_QNET_STEP_MAX_PARTIALS; 0 for a bad dim_ff or n_layers.
 * Arguments are checked before any device call: a null or misaligned pointer, dim_ff not a multiple of 32, n_layers outside
 * 1 .. 64, step 0, an lr, beta1, beta2, eps or weight_decay that is negative or not finite, beta1 or beta2 >= 1, max_norm NaN or
 * <= 0 return G2048_ERR_ARG. */
#define G2048_QNET_STEP_MAX_PARTIALS 1024
G2048_API size_t g2048_qnet_step_workspace(int dim_ff, int n_layers);
G2048_API int g2048_qnet_adamw_step(float *plain, float *grad, float *exp_avg, float *exp_avg_sq, int dim_ff, int n_layers, float lr,
                          float beta1, float beta2, float eps, float weight_decay, float max_norm, uint64_t step, float *norm_out,
                          void *workspace, void *stream);

/* ---- the PPO update's loss and gradient pass (agents/ppo_agent.py:357-400) --------------------------------------------------
 * The lines of PPOAgent.update() that need the networks in TRAINING mode, for the reference's ActorNetwork / CriticNetwork
 * (16-256-128-64-{4|1}): h1 = relu(fc1 x), b1 = BN1(h1), h2 = relu(fc2 b1), b2 = BN2(h2), h3 = relu(fc3 b2), z = fc4 h3. The
 * BatchNorms use the batch mean and the biased variance over the n rows (eps 1e-5); given a running-statistics buffer they move
 * it by momentum 0.1 towards the batch mean and the UNBIASED variance, as torch does. For n == 1 the reference's forward skips
 * both BatchNorms, and so does this: their gradients are written as 0 and the running statistics are untouched. The reference
 * runs these lines with its dropout live (nn.Dropout(0.2) on b1 and b2); g2048_ppo_forward_train and g2048_ppo_loss_grad leave
 * it out (p = 0), the *_dropout entry points below apply it. f32 only. The inputs are the float observations PPOAgent.update
 * builds (states float32 [n][16], 16-byte aligned), not packed boards.
 *
 * One network's parameters are one PLAIN f32 buffer of 46272 + 65 * n_out floats (n_out 4: actor, 1: critic), torch's row-major
 * [out][in], back to back:
 *     fc1.weight [256][16]  fc1.bias [256]  bn1.weight [256]  bn1.bias [256]  fc2.weight [128][256]  fc2.bias [128]
 *     bn2.weight [128]  bn2.bias [128]  fc3.weight [64][128]  fc3.bias [64]  fc4.weight [n_out][64]  fc4.bias [n_out]
 * A gradient buffer has the same layout. A running-statistics buffer is 768 floats: bn1.running_mean [256], bn1.running_var
 * [256], bn2.running_mean [128], bn2.running_var [128]. Plain and gradient buffers are 16-byte aligned.
 *
 *   g2048_ppo_train_workspace   bytes of `workspace` for n rows (device memory, 16-byte aligned, contents irrelevant before and
 *       meaningless after); 0 for n == 0 or n > G2048_PPO_BATCH_MAX. Non-decreasing in n. One size serves the three calls below.
 *   g2048_ppo_forward_train   one network's training-mode forward: out = softmax probabilities float32 [n][4] (16-byte aligned)
 *       for n_out 4, values float32 [n][1] for n_out 1. The running statistics are updated iff running_or_null is given.
 *   g2048_ppo_advantages   :368-373 in one launch: returns_out = rewards + gamma * next_values * (1 - dones), adv = returns_out -
 *       values, and for n > 1 adv_out = (adv - mean) / (std + 1e-8) with torch's unbiased std; mean and variance are one block's
 *       fixed-order sums. For n == 1 adv_out = adv.
 *   g2048_ppo_loss_grad   one epoch body :378-400 up to backward(): both training-mode forwards (each network's running statistics
 *       updated iff its pointer is given), then with p = softmax(z_actor) and Categorical(probs = p) evaluated as torch evaluates
 *       it in f32 (q = p / sum p; log q taken of q clamped to [eps, 1 - eps], eps = 2^-23; no gradient through a binding clamp):
 *         ratio = exp(log q[a] - old_log_probs), a = actions[i] & 3 (int64; nothing is read out of bounds);
 *         actor_loss = -mean(min(ratio A, clamp(ratio, 1 - clip_epsilon, 1 + clip_epsilon) A)), A = advantages, with torch's
 *           subgradients: a tie's gradient is split in halves, clamp passes it on the closed range;
 *         value_loss = mean((v - returns)^2);  entropy = mean(-sum q log q);
 *         loss = actor_loss + value_coef * value_loss - entropy_coef * entropy;
 *         loss_out = {loss, actor_loss, value_loss, entropy}. A NaN loss is reported there; the reference's `continue` on it is
 *           the caller's decision.
 *       grad_actor_out and grad_critic_out = d loss / d parameter, in the plain layout, OVERWRITTEN, never accumulated into.
 *       One phase per launch on `stream`: fc1 and the products fc2, fc3, dX and dW / db on the f32 matrix cores, BatchNorm forward
 *       and backward and the heads (fc4, the loss, its derivative) on the VALU. No atomics, no split-K across blocks: every
 *       output element is one fixed-order accumulation, so two calls give the same bits. Nothing past row n or past the stated
 *       sizes is read or written.
 *
 * Dropout (the reference's training-mode forwards; RNG domain 11 of DESIGN.md "RNG"). With probability p, b1 and b2 (for n == 1,
 * where the BatchNorms are skipped: h1 and h2) are multiplied element by element by m before fc2 / fc3 read them. For the library
 * call with index `call_index`, (k0, k1) = rng_keys(seed, 11, call_index); element (row, feature) of site s (0: b1, F = 256; 1: b2,
 * F = 128) of network w (0 actor, 1 critic) draws h = rng_draw(k0, k1, id, 0), id = ((uint64)(2 w + s) << 32) | (row * F + feature),
 * and is kept iff h >= T, T = (uint32) floor(p * 2^32) formed in double; m = (float)(1.0 / (1.0 - p)) if kept, else 0.0f. It is a
 * multiplication both ways (y = x * m, dx = dy * m), as in torch: a NaN or an infinity in a dropped position becomes NaN. The
 * backward regenerates m; no mask is stored and the workspace is the same. p is a double, 0 <= p < 1 and finite.
 *   g2048_ppo_forward_train_dropout   g2048_ppo_forward_train with dropout p on the masks of network `net` (0 or 1, whatever
 *       n_out is: the critic's forwards of the advantages block pass 1).
 *   g2048_ppo_loss_grad_dropout   g2048_ppo_loss_grad with p_actor on the actor (w = 0) and p_critic on the critic (w = 1); both
 *       networks share call_index. Still one fixed-order accumulation per output element: two calls with the same seed and
 *       index give the same bits.
 *   g2048_ppo_dropout_mask   keep_out uint8 [n][F] = 1 where the element of (net, site) is kept, written through the function the
 *       two passes draw with; for callers who reproduce a step, and for tests. 1 <= n <= G2048_PPO_BATCH_MAX.
 *   With p == 0 (p_actor == p_critic == 0) the two passes launch exactly the kernels of the entry points without dropout and give
 *   their bits. A network with p == 0 next to one with p > 0 is the pass without dropout for that network.
 *
 * A ReLU's backward, in all of these passes, is torch's threshold_backward: the gradient is zeroed where the ReLU's output is <= 0,
 * so it passes where the output is a NaN (a non-finite row of `states`), and each gradient tensor is then non-finite where stock
 * torch's is. One exception: n == 1 in a network WITHOUT dropout. There the two hidden ReLUs' backward is the mask of the shared dX
 * product (the Q-network's kernel), which keeps the gradient where the output is > 0 and so zeroes it at a NaN; the loss parts are
 * NaN all the same, which is what the optimiser's gate reads. n == 1 with p > 0 and every n > 1 follow torch.
 *
 * 1 <= n <= G2048_PPO_BATCH_MAX (the batch statistics are the whole batch's: a larger n is refused, not truncated); n == 0
 * returns G2048_OK and does nothing. Arguments are checked before any device call: a null or misaligned pointer, n too large,
 * n_out other than 4 or 1, net or site other than 0 or 1, a clip_epsilon, value_coef or entropy_coef that is negative or not
 * finite, a p that is negative, >= 1 or not finite return G2048_ERR_ARG. */
#define G2048_PPO_BATCH_MAX 4096
G2048_API size_t g2048_ppo_train_workspace(size_t n);
G2048_API int g2048_ppo_forward_train(const float *states, const float *plain, float *running_or_null, int n_out, float *out, size_t n,
                            void *workspace, void *stream);
G2048_API int g2048_ppo_advantages(const float *values, const float *next_values, const float *rewards, const float *dones, float gamma,
                         float *returns_out, float *adv_out, size_t n, void *stream);
G2048_API int g2048_ppo_loss_grad(const float *states, const int64_t *actions, const float *old_log_probs, const float *advantages,
                        const float *returns, const float *plain_actor, const float *plain_critic, float *running_actor_or_null,
                        float *running_critic_or_null, float clip_epsilon, float value_coef, float entropy_coef, size_t n,
                        float *grad_actor_out, float *grad_critic_out, float *loss_out, void *workspace, void *stream);
G2048_API int g2048_ppo_forward_train_dropout(const float *states, const float *plain, float *running_or_null, int n_out, int net, double p,
                                    uint64_t seed, uint64_t call_index, float *out, size_t n, void *workspace, void *stream);
G2048_API int g2048_ppo_loss_grad_dropout(const float *states, const int64_t *actions, const float *old_log_probs, const float *advantages,
                                const float *returns, const float *plain_actor, const float *plain_critic, float *running_actor_or_null,
                                float *running_critic_or_null, float clip_epsilon, float value_coef, float entropy_coef, double p_actor,
                                double p_critic, uint64_t seed, uint64_t call_index, size_t n, float *grad_actor_out,
                                float *grad_critic_out, float *loss_out, void *workspace, void *stream);
G2048_API int g2048_ppo_dropout_mask(uint64_t seed, uint64_t call_index, int net, int site, double p, uint8_t *keep_out, size_t n,
                           void *stream);

/* ---- the PPO update's loss gate, gradient clipping and Adam step (agents/ppo_agent.py:403-416) ------------------------------
 * What an epoch of PPOAgent.update() does after backward(), for the actor and the critic TOGETHER: `if torch.isnan(loss):
 * continue`, clip_grad_norm_(parameters, max_norm) on each network and torch.optim.Adam.step() on each network. The parameters
 * are the two PLAIN f32 buffers (layout above: 46532 floats for the actor, 46337 for the critic), the gradients the buffers
 * g2048_ppo_loss_grad fills, the moment estimates two more buffers per network of the same layout that start as zeros. All eight
 * are 16-byte aligned; the critic's count is 1 mod 4, so its buffers end in a 16-byte group of one float.
 * `counters` is four int64 on the device, 8-byte aligned, that start as zeros and belong to the pair of networks:
 *     {actor steps applied, critic steps applied, calls skipped for a NaN loss, calls skipped for a gradient norm that is not finite}
 *
 *   g2048_ppo_adam_step   two launches on `stream`, no host synchronisation and no host decision:
 *       1. prepare: ONE block of 1,024 threads. Each network's gradient norm: thread t adds grad[i]^2 over the 16-byte groups t,
 *          t + 1,024, .. in order, then the wavefront's butterfly and the sixteen wavefronts' sums pairwise, all in f64, in an order
 *          that depends on the float count alone; norms_out = {(float)sqrt(actor's sum), (float)sqrt(critic's sum)}, written on
 *          EVERY call, a skipped one included. Then one thread decides. The call is SKIPPED if
 *            - loss_or_null is given and loss_or_null[0] is a NaN (the reference's rule, isnan only: a +inf loss over finite
 *              gradients is applied; loss_or_null[1..] is never read): counters[2] += 1; or else
 *            - EITHER network's norm is not finite (an inf or a NaN in a gradient; stock torch would write NaN into every weight
 *              of that network, and an update that reaches one network and not the other is of no use): counters[3] += 1.
 *          A skipped call writes nothing else: all eight buffers keep their bits and counters[0], counters[1] stay. Otherwise
 *          counters[0] and counters[1] go up by one, and for each network, with t = its counter's new value, the thread forms in
 *          f64 bc1 = 1 - beta1^t and bc2 = 1 - beta2^t, and passes on lr / bc1, sqrt(bc2) (rounded to f32) and the clip coefficient
 *          c = min(1, max_norm / (norm + 1e-6)), evaluated as torch evaluates it in f32: the reciprocal of norm + 1e-6, times
 *          max_norm; max_norm = +inf: no clipping. The step number lives on the device because the host never learns of a skipped
 *          call, and a skipped call must not advance the bias correction (the reference's `continue` does not reach
 *          optimizer.step()); this is the difference from g2048_qnet_adamw_step, whose caller counts.
 *       2. update: one grid over both networks; every block reads those scalars and returns at once on a skip. Otherwise, for
 *          every element, with its network's own lr, eps and c:
 *              g = grad[i] * c;  grad[i] = g                      (grad is left clipped, as clip_grad_norm_ leaves it)
 *              m = m + (g - m) * (1 - beta1)
 *              v = v * beta2 + (g * g) * (1 - beta2)
 *              p = p - (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps))
 *          every operation rounded to f32 on its own, in the order of torch's single-tensor Adam (g2048_qnet_adamw_step's lines
 *          without weight decay). 1 - beta1 and 1 - beta2 are formed on the host in f64 from the shortest decimal that rounds to
 *          the float given, as there.
 *       No atomics, no block waits on another; the counters are read and written by the one block of the first launch alone. Two
 *       calls from the same state give the same bits. Nothing outside the eight buffers, the counters, norms_out[0..1] and the
 *       workspace is written.
 *   g2048_ppo_step_workspace   bytes of `workspace` (device memory, 16-byte aligned, contents irrelevant before and meaningless
 *       after): the prepared scalars.
 * Arguments are checked before any device call: a null pointer (other than loss_or_null) or a misaligned one, an lr, beta or eps
 * that is negative or not finite, a beta >= 1, max_norm NaN or <= 0 return G2048_ERR_ARG. */
G2048_API size_t g2048_ppo_step_workspace(void);
G2048_API int g2048_ppo_adam_step(float *plain_actor, float *grad_actor, float *exp_avg_actor, float *exp_avg_sq_actor,
                        float *plain_critic, float *grad_critic, float *exp_avg_critic, float *exp_avg_sq_critic,
                        const float *loss_or_null, int64_t *counters, float lr_actor, float lr_critic, float beta1, float beta2,
                        float eps_actor, float eps_critic, float max_norm, float *norms_out, void *workspace, void *stream);
#ifdef __cplusplus
}
#endif
#endif
