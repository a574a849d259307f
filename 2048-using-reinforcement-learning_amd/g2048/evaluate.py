"""Batched evaluation driver: many beam-search games played to completion, resident on the GPU.

Device-resident version of the reference's evaluation loops --
`run_evaluation.evaluate_beam_search` (run_evaluation.py:48-130) and
`evaluate_beam_search.run_game / run_evaluation` (evaluate_beam_search.py:16-217): every game does
`action = agent.get_action(state)` (no caller mask, so the agent's own validity check applies,
run_evaluation.py:62) then `env.step(action)` until done or the move cap (5000, run_evaluation.py:67).
Here all games advance together: one `g2048_beam_get_action` launch (one wavefront per game) and one
`g2048_step` launch per move, no host round trip except an "all finished?" poll every `check_every` moves.
Finished games stay in the batch as no-ops (their counters are frozen), so ids -- and therefore every random
draw -- never change: game g at move t always uses draws (seed, BEAM|STEP, t, game_id_base + g).

The result dict has the keys of both reference drivers (scores, highest_tiles, moves, valid_moves,
invalid_moves, milestones, best_games, final_boards, best_board, best_score, best_game_idx) and
`save_overall_results` writes the reference's overall_results.json schema (evaluate_beam_search.py:198-214).

Per-game histories (`histories=`): the reference's `run_game` also returns `board_history`, `max_tiles_history` and
`scores_history` (evaluate_beam_search.py:44-50, :72-75, :88-97), writes them to `game_{i}_data.json` for the games that
reached 2048 (:185-196), and `train.py` keeps every episode's move-set (`moveset`, :51, :67) and writes the best ones to
`*_best_moveset_tile_N.txt` (:140-142). The fused kernel keeps ONE byte per move (the action); since every spawn is a
counter-based draw keyed by (seed, move, game id), replaying those bytes on the device (`g2048_replay_games`) rebuilds every
intermediate board, score and max tile of the games asked for -- `results["games"][i]` has the reference's `run_game` keys,
`save_game_data` / `save_moveset` write the reference's two file formats.

`evaluate_policy` is the same for a PPO actor (a DevicePolicy): the games of train.py / play.py, every game to its end in one
`g2048_play_policy_games` launch, with the same result dict plus each game's summed env reward. A DeviceTransformerPolicy plays
the same games with the transformer's probabilities (`g2048_play_tpolicy_games`). `evaluate_qnet` plays the hybrid agent's
Q-network (a DeviceQNetwork) with select_action's epsilon-greedy rule (`g2048_play_qnet_games`).
"""
import json
import time
import warnings

import torch

from . import _lib as L
from . import ops
from .vec import VecGame2048

MILESTONES = (64, 128, 256, 512, 1024, 2048, 4096, 8192)      # evaluate_beam_search.py:42-43 (fixed in the kernel)


def evaluate_beam_search(num_games=4096, beam_width=20, search_depth=30, seed=0x2048, max_moves=5000,
                         device="cuda", game_id_base=0, check_every=64, early_game_threshold=512,
                         mid_game_threshold=1024, fixed_down=False, use_graph=True, fused=True, one_phase=False, _table_only=False,
                         tuning=None, histories=None):
    """fused=True (default): every game is played start to finish by its own wavefront in one kernel launch
    (`g2048_play_games`; helper wavefronts of that launch pre-compute decisions for the last games, one_phase=True turns
    them off -- same games). fused=False: the step-by-step loop (one beam launch + one step launch + bookkeeping per move for
    the whole batch; with use_graph=True a captured hipGraph of one move is replayed). All three produce identical games.
    tuning = (helpers, games_left, stuck, wait_us): explicit helper-wavefront parameters (ops.play_games; measurements, tests).
    histories: None, or which games also get their per-move histories (results["games"][i]: board_history, scores_history,
    max_tiles_history, moveset, ... -- the dict evaluate_beam_search.run_game returns): "best5" (results["best_games"]),
    "high_tile" (every game that reached 2048, the ones the reference writes game_N_data.json for), "all", or an iterable of
    game indices. Fused driver only: the kernel records one action byte per move and the asked games are replayed on the device."""
    dev = torch.device(device)
    n = int(num_games)
    if histories is not None and not fused:
        raise ValueError("g2048.evaluate_beam_search: histories need the fused driver (fused=True)")
    t_start = time.perf_counter()
    env = VecGame2048(n, device=dev, seed=seed, id_base=game_id_base)
    boards0 = env.boards.clone() if histories is not None else None
    actions = None
    alive = torch.ones(n, dtype=torch.uint8, device=dev)
    moves = torch.zeros(n, dtype=torch.int32, device=dev)
    valid_cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    invalid_cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    ms_move = torch.full((n, len(MILESTONES)), -1, dtype=torch.int32, device=dev)
    expanded_sum = torch.zeros(n, dtype=torch.int64, device=dev)
    t = 0
    graph = None
    if fused:
        res = ops.play_games(env.boards, env.scores, beam_width, search_depth, max_moves, early_game_threshold,
                             mid_game_threshold, seed, game_id_base, fixed_down, one_phase, tuning=tuning,
                             want_actions=histories is not None)
        alive, moves, valid_cnt, invalid_cnt = res["alive"], res["moves"], res["valid_moves"], res["invalid_moves"]
        ms_move, expanded_sum = res["milestone_move"], res["expanded"]
        actions = res.get("actions")
        t = max_moves
    elif use_graph:
        # One move = [keys_advance, beam, step (in place), track], all reading their RNG keys / move index from a device
        # key block, captured once into a hipGraph and replayed per move: no per-move host work besides the replay.
        kb = ops.KeyBlock(seed, 0, dev)
        out = (torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.float32, device=dev),
               torch.empty(n, dtype=torch.int32, device=dev))

        def one_move():
            kb.advance()
            ops.beam_get_action(env.boards, beam_width, search_depth, None, early_game_threshold, mid_game_threshold,
                                game_id_base=game_id_base, fixed_down=fixed_down, keyblock=kb, out=out)
            ops.step(env.boards, out[0], env.scores, 0, 0, game_id_base, out=env.boards, reward=env.reward, flags=env.flags,
                     keyblock=kb)
            ops.track_episodes(env.flags, alive, moves, valid_cnt, invalid_cnt, ms_move, 0, out[2], expanded_sum, keyblock=kb)
        # The warm-up move below really executes (capture does not), so the state is snapshotted first -- on the current
        # stream, BEFORE the side stream is made to wait for it, so the snapshot is ordered ahead of the warm-up -- and
        # restored afterwards whether or not the capture succeeded: the loop always starts from move 0.
        tracked = (env.boards, env.scores, alive, moves, valid_cnt, invalid_cnt, ms_move, expanded_sum, kb.counter)
        state = [x.clone() for x in tracked]
        cur = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(cur)
        try:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                one_move()                      # warm-up outside capture
                side.synchronize()
                with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
                    one_move()
        except Exception as exc:                # noqa: BLE001 -- capture unavailable: plain launches, same games
            warnings.warn("g2048.evaluate_beam_search: hipGraph capture failed (%s: %s); falling back to one launch "
                          "sequence per move" % (type(exc).__name__, exc), RuntimeWarning, stacklevel=2)
            graph = None
            torch.cuda.synchronize(dev)
        cur.wait_stream(side)
        for dst, src in zip(tracked, state):
            dst.copy_(src)                      # rewind to move 0
    while t < max_moves:
        if graph is not None:
            graph.replay()
        else:
            actions, _, expanded = ops.beam_get_action(env.boards, beam_width, search_depth, None, early_game_threshold,
                                                       mid_game_threshold, seed, t, game_id_base, fixed_down,
                                                       want_expanded=True)
            env.step(actions)
            # evaluate_beam_search.py:42-64 for every game, one kernel
            ops.track_episodes(env.flags, alive, moves, valid_cnt, invalid_cnt, ms_move, t, expanded, expanded_sum)
        t += 1
        if t % check_every == 0 and not bool(alive.any()):
            break
    expanded_total = expanded_sum.sum()
    torch.cuda.synchronize(dev)
    elapsed = time.perf_counter() - t_start

    table = _game_table(env.scores, moves, valid_cnt, invalid_cnt, alive, expanded_sum, ms_move, env.boards)
    if _table_only:
        return table.cpu().numpy()
    results = results_from_table(table.cpu().numpy(), elapsed, beam_width, search_depth, seed, max_moves)
    if histories is not None:
        results["games"] = game_histories(results, histories, boards0, actions, moves, seed, game_id_base)
    return results


def _game_table(scores, moves, valid, invalid, alive, expanded, milestone_move, boards):
    """One int64 row per game: score, moves, valid, invalid, alive, expanded (None: 0), 8 milestone moves, 16 tiles."""
    n = boards.shape[0]
    if expanded is None:
        expanded = torch.zeros(n, dtype=torch.int64, device=boards.device)
    return torch.cat([scores.to(torch.int64)[:, None], moves.to(torch.int64)[:, None], valid.to(torch.int64)[:, None],
                      invalid.to(torch.int64)[:, None], alive.to(torch.int64)[:, None], expanded[:, None],
                      milestone_move.to(torch.int64), ops.unpack(boards).to(torch.int64).reshape(n, 16)], dim=1)


POLICY_MODES = ("masked", "unmasked", "greedy")


def _evaluate_net(dev, fused, play_fused, play_stepwise, params, game_id_base, histories):
    """evaluate_policy and evaluate_qnet from their argument checks on: play_fused(env, want_actions) / play_stepwise(env) play
    the games of `env` to their ends and return the per-game dict of ops.play_policy_games; params is the "parameters" entry."""
    n, seed = params["num_games"], params["seed"]
    t_start = time.perf_counter()
    env = VecGame2048(n, device=dev, seed=seed, id_base=game_id_base)
    boards0 = env.boards.clone() if histories is not None else None
    res = play_fused(env, histories is not None) if fused else play_stepwise(env)
    torch.cuda.synchronize(dev)
    elapsed = time.perf_counter() - t_start
    table = _game_table(env.scores, res["moves"], res["valid_moves"], res["invalid_moves"], res["alive"], None, res["milestone_move"],
                        env.boards)
    results = policy_results_from_table(table.cpu().numpy(), res["reward_sum"].cpu().numpy(), elapsed, params)
    if histories is not None:
        results["games"] = game_histories(results, histories, boards0, res["actions"], res["moves"], seed, game_id_base)
    return results


def _is_transformer(policy):
    from .tpolicy import DeviceTransformerPolicy
    return isinstance(policy, DeviceTransformerPolicy)


def evaluate_policy(policy, num_games=4096, max_moves=2000, mode="masked", seed=0x2048, game_id_base=0, device=None,
                    fused=True, histories=None, max_waves=0):
    """Complete games of a PPO actor (a g2048.DevicePolicy; its critic, if any, is not used): the games of train.py:54-90
    (mode="masked": agent.get_action(state, env.get_valid_moves()), max_steps = 2000) or play.py:44-68 ("unmasked":
    agent.get_action(state)), or the argmax over the valid moves ("greedy"). The network sees one board at a time, as in the
    reference, so it plays with the weights DevicePolicy uses for a batch of one row (actor.blob(1): no BatchNorm for the
    reference's fc/bn layout). Game g starts from VecGame2048's reset of global id game_id_base + g.

    fused=True: every game is played to the end in ONE launch (g2048_play_policy_games; max_waves = its wavefront count, 0 =
    as many as the chip holds). fused=False: the step-by-step loop of existing launches -- policy_forward, sample_actions
    (greedy: torch's argmax), step, track_episodes -- over the whole batch until every game has ended: the yardstick; the games
    are identical. Returns evaluate_beam_search's result dict (scores, highest_tiles, moves, valid / invalid moves, milestones,
    best_games, final_boards, best_*, unfinished, total_moves, elapsed_s, summary) plus "episode_rewards" (the f64 env rewards
    of each game summed in move order: train.py's episode_reward, play.py's total_reward); "parameters" holds mode,
    precision, max_moves, num_games and seed. histories: as in evaluate_beam_search (fused driver only).

    policy may also be a g2048.DeviceTransformerPolicy: the same games, modes and result dict with the transformer's
    probabilities (its value head is not used). fused=True is ONE g2048_play_tpolicy_games launch (max_waves = its BLOCK
    count, 16 games in flight each; 0 = as many as the chip holds); fused=False the loop of tpolicy_forward(want_value=False),
    valid_moves, sample_actions / argmax, step and track_episodes."""
    transformer = _is_transformer(policy)
    if not transformer and (not hasattr(policy, "actor") or not hasattr(policy.actor, "blob")):
        raise TypeError("g2048.evaluate_policy: policy must be a g2048.DevicePolicy or a g2048.DeviceTransformerPolicy")
    if mode not in POLICY_MODES:
        raise ValueError("g2048.evaluate_policy: mode must be one of %s" % (POLICY_MODES,))
    if int(max_moves) < 1:
        raise ValueError("g2048.evaluate_policy: max_moves must be at least 1")
    if histories is not None and not fused:
        raise ValueError("g2048.evaluate_policy: histories need the fused driver (fused=True)")
    dev = policy.device
    if device is not None and ops._dev_index(torch.device(device)) != ops._dev_index(dev):
        raise ValueError("g2048.evaluate_policy: the policy lives on %s, not %s" % (dev, device))
    n, max_moves = int(num_games), int(max_moves)
    precision = policy.precision
    blob = policy.packed if transformer else policy.actor.blob(1)
    if transformer:
        net, play, units = (policy.dim_ff, policy.n_layers), ops.play_tpolicy_games, "max_blocks"

        def forward(boards, probs):
            ops.tpolicy_forward(boards, blob, *net, precision, probs=probs, want_value=False)
    else:
        net, play, units, forward = (), ops.play_policy_games, "max_waves", None
    return _evaluate_net(
        dev, fused,
        lambda env, want_actions: play(env.boards, env.scores, blob, *net, precision, max_moves, mode, seed, game_id_base,
                                       want_rewards=True, want_actions=want_actions, **{units: max_waves}),
        lambda env: _play_policy_stepwise(env, blob, precision, max_moves, mode, seed, game_id_base, forward=forward),
        {"mode": mode, "precision": precision, "max_moves": max_moves, "num_games": n, "seed": seed}, game_id_base, histories)


def evaluate_qnet(qnet, num_games=4096, max_moves=2000, epsilon=0.0, seed=0x2048, game_id_base=0, device=None, fused=True,
                  histories=None, max_waves=0, use_beam_search=False, beam_width=15, search_depth=30, beam_search_threshold=64):
    """Complete games of the hybrid agent's Q-network (a g2048.DeviceQNetwork): the reference's evaluate_agent
    (hybrid.py:1176-1210), select_action -> env.step until the game is over or max_moves moves were made (2000: train_agent's
    max_steps). epsilon is select_action's (evaluate_agent runs at 0.01; 0 = the exploit action alone). Game g starts from
    VecGame2048's reset of global id game_id_base + g.

    use_beam_search=True is the reference's own configuration (DQNAgent sets it, with beam_width 15, search_depth 30,
    beam_search_threshold 64, gamma 0.99): where its beam_search plans -- max tile >= the threshold and at least 8 tiles -- the
    exploit action is that search's decision. The reference's search never goes past its first level (include/g2048.h), so at
    search_depth >= 2 it is a closed form of the board that consults no network, and the network decides only boards below the
    threshold or with fewer than 8 tiles. fused=True is then ONE g2048_play_qnet_beam_games launch, fused=False the loop with
    qnet_beam_actions in place of qnet_select_actions. search_depth 1 values every candidate with the network (the draws of its
    candidates keyed by (seed, SIMULATE, move, game id)) and runs only with fused=False. The default, False, is select_action
    with use_beam_search = False.

    fused=True: every game is played to the end in ONE launch (g2048_play_qnet_games; max_waves = its wavefront count, 32
    games in flight each, 0 = as many as the chip holds). fused=False: the step-by-step loop of the launches that exist apart
    from it -- qnet_forward with actions, qnet_select_actions when epsilon > 0, step, track_episodes -- over the whole batch
    until every game has ended: the yardstick; the games are identical. Returns evaluate_policy's result dict, episode_rewards
    included; "parameters" holds epsilon, precision, max_moves, num_games and seed, as before, and with the search also
    use_beam_search, beam_width, search_depth, beam_search_threshold and gamma. histories: as in evaluate_beam_search (fused driver only)."""
    from .qnet import DeviceQNetwork
    if not isinstance(qnet, DeviceQNetwork):
        raise TypeError("g2048.evaluate_qnet: qnet must be a g2048.DeviceQNetwork")
    epsilon = float(epsilon)
    if not 0.0 <= epsilon <= 1.0:
        raise ValueError("g2048.evaluate_qnet: epsilon must lie in [0, 1]")
    if int(max_moves) < 1:
        raise ValueError("g2048.evaluate_qnet: max_moves must be at least 1")
    if histories is not None and not fused:
        raise ValueError("g2048.evaluate_qnet: histories need the fused driver (fused=True)")
    beam = None
    if use_beam_search:
        beam = (int(beam_width), int(search_depth), int(beam_search_threshold))
        if not 1 <= beam[0] <= 64:
            raise ValueError("g2048.evaluate_qnet: beam_width must lie in 1 .. 64")
        if beam[1] < 1:
            raise ValueError("g2048.evaluate_qnet: search_depth must be at least 1")
        if beam[2] < 1:
            raise ValueError("g2048.evaluate_qnet: beam_search_threshold (a tile value) must be at least 1")
        if beam[1] == 1 and fused:
            raise ValueError("g2048.evaluate_qnet: search_depth 1 asks the network about every candidate and is not played in one "
                             "launch; it runs with fused=False")
    dev = qnet.device
    if device is not None and ops._dev_index(torch.device(device)) != ops._dev_index(dev):
        raise ValueError("g2048.evaluate_qnet: the network lives on %s, not %s" % (dev, device))
    n, max_moves = int(num_games), int(max_moves)
    precision, blob, dim_ff, n_layers = qnet.precision, qnet.packed, qnet.dim_ff, qnet.n_layers
    params = {"epsilon": epsilon, "precision": precision, "max_moves": max_moves, "num_games": n, "seed": seed}
    if beam is None:
        def play(env, want_actions):
            return ops.play_qnet_games(env.boards, env.scores, blob, dim_ff, n_layers, precision, max_moves, epsilon, seed, game_id_base,
                                       want_rewards=True, want_actions=want_actions, max_waves=max_waves)
    else:
        params.update(use_beam_search=True, beam_width=beam[0], search_depth=beam[1], beam_search_threshold=beam[2], gamma=BEAM_GAMMA)

        def play(env, want_actions):
            return ops.play_qnet_beam_games(env.boards, env.scores, blob, dim_ff, n_layers, precision, max_moves, epsilon, *beam, seed,
                                            game_id_base, want_rewards=True, want_actions=want_actions, max_waves=max_waves)
    return _evaluate_net(
        dev, fused, play,
        lambda env: _play_policy_stepwise(env, blob, precision, max_moves, None, seed, game_id_base,
                                          act=qnet_stepwise_act(blob, dim_ff, n_layers, precision, n, dev, epsilon, seed, game_id_base,
                                                                beam)),
        params, game_id_base, histories)


def evaluate_expectimax(num_games=4096, depth=2, max_moves=5000, seed=0x2048, game_id_base=0, fused=True, device=None,
                        early_game_threshold=512, mid_game_threshold=1024, histories=None, max_waves=0):
    """Complete games of the expectimax agent (ops.expectimax_actions: the expectation over all spawn successors, `depth` plies,
    1..3, the beam agent's leaf heuristic): decide -> env step until the game is over or max_moves moves were made. Game g starts
    from VecGame2048's reset of global id game_id_base + g; the agent draws nothing, so `seed` is the env's alone.

    fused=True: every game is played to the end in ONE launch (g2048_play_expectimax_games; max_waves = its wavefront count,
    one game in flight each, 0 = as many as the chip holds). fused=False: the move-by-move loop of the launches that exist apart
    from it -- expectimax_actions, step, track_episodes -- over the whole batch until every game has ended: the yardstick; the
    games are identical. Returns evaluate_policy's result dict, episode_rewards included; "parameters" holds depth, the two
    thresholds, max_moves, num_games and seed. histories: as in evaluate_beam_search (fused driver only)."""
    n, depth, max_moves = int(num_games), int(depth), int(max_moves)
    early, mid = int(early_game_threshold), int(mid_game_threshold)
    ops._check_expectimax(depth, early, mid)
    if max_moves < 1:
        raise ValueError("g2048.evaluate_expectimax: max_moves must be at least 1")
    if histories is not None and not fused:
        raise ValueError("g2048.evaluate_expectimax: histories need the fused driver (fused=True)")
    dev = torch.device("cuda" if device is None else device)

    def act(boards, t):
        return ops.expectimax_actions(boards, depth, None, False, early, mid)

    return _evaluate_net(
        dev, fused,
        lambda env, want_actions: ops.play_expectimax_games(env.boards, env.scores, depth, max_moves, early, mid, seed, game_id_base,
                                                            want_rewards=True, want_actions=want_actions, max_waves=max_waves),
        lambda env: _play_policy_stepwise(env, None, None, max_moves, None, seed, game_id_base, act=act),
        {"depth": depth, "early_game_threshold": early, "mid_game_threshold": mid, "max_moves": max_moves, "num_games": n, "seed": seed},
        game_id_base, histories)


BEAM_GAMMA = 0.99           # DQNAgent's gamma (hybrid.py:769); it enters the search only at search_depth 1


def qnet_stepwise_act(blob, dim_ff, n_layers, precision, n, device, epsilon, seed, game_id_base, beam=None):
    """The `act` of _play_policy_stepwise for the Q-network, built only from launches that exist apart from the game kernel:
    qnet_forward with its exploit actions and, when epsilon > 0, qnet_select_actions with step_index = the move.
    beam = (beam_width, search_depth, threshold): use_beam_search = True -- qnet_forward, then qnet_beam_actions; at
    search_depth 1 qnet_beam_expand and the forward on the n x 32 candidate boards come between them."""
    q = torch.empty((n, 4), dtype=torch.float32, device=device)
    actions = torch.empty(n, dtype=torch.uint8, device=device)
    explored = torch.empty(n, dtype=torch.uint8, device=device)
    if beam is None:
        def act(boards, t):
            ops.qnet_forward(boards, blob, dim_ff, n_layers, precision, q=q, actions=actions)
            if epsilon > 0:
                ops.qnet_select_actions(q, boards, epsilon, seed, t, game_id_base, actions=actions, explored=explored)
            return actions
        return act
    planned = torch.empty(n, dtype=torch.uint8, device=device)
    depth_one = beam[1] == 1
    if depth_one:
        succ = torch.empty((n, 32, 16), dtype=torch.uint8, device=device)
        count = torch.empty((n, 4), dtype=torch.uint8, device=device)
        succ_q = torch.empty((n, 32, 4), dtype=torch.float32, device=device)

    def act_beam(boards, t):
        ops.qnet_forward(boards, blob, dim_ff, n_layers, precision, q=q)
        if depth_one:
            ops.qnet_beam_expand(boards, seed, t, game_id_base, succ=succ, count=count)
            ops.qnet_forward(succ.view(n * 32, 16), blob, dim_ff, n_layers, precision, q=succ_q.view(n * 32, 4))
        ops.qnet_beam_actions(q, boards, succ_q if depth_one else None, *beam, BEAM_GAMMA, epsilon, seed, t, game_id_base,
                              actions=actions, planned=planned, explored=explored)
        return actions
    return act_beam


def policy_results_from_table(table, episode_rewards, elapsed, parameters):
    """evaluate_policy's result dict from the per-game table (evaluate_beam_search's columns, no expansions) and the f64
    reward sums."""
    results = results_from_table(table, elapsed, None, None, parameters["seed"], parameters["max_moves"], parameters=parameters)
    results["episode_rewards"] = [float(r) for r in episode_rewards]
    results["summary"] = summarize(results)
    return results


def _play_policy_stepwise(env, blob, precision, max_moves, mode, seed, game_id_base, check_every=16, forward=None, act=None):
    """The unfused yardstick of g2048_play_policy_games: one policy_forward, one action launch (sample_actions with step_index
    = t, or torch's argmax), one step and one track_episodes per move for the whole batch. A finished game is over (no move
    changes its board), so stepping it again changes nothing; its counters and reward sum are frozen by `alive`.
    forward: forward(boards, probs) fills probs (float32 (n,4)) for the boards with one launch; None = the PPO actor's
    policy_forward on `blob`. With the transformer's forward this is the yardstick of g2048_play_tpolicy_games.
    act: act(boards, t) returns the uint8 (n,) actions of move t itself, in place of forward, mode and the action launch (blob,
    precision and mode are then unused): with the Q-network's forward and select launches this is the yardstick of
    g2048_play_qnet_games."""
    if forward is None and act is None:
        def forward(boards, probs):
            ops.policy_forward(boards, blob, None, precision, probs=probs)
    n, dev = env.n, env.device
    alive = torch.ones(n, dtype=torch.uint8, device=dev)
    moves = torch.zeros(n, dtype=torch.int32, device=dev)
    valid_cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    invalid_cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    ms_move = torch.full((n, len(MILESTONES)), -1, dtype=torch.int32, device=dev)
    reward_sum = torch.zeros(n, dtype=torch.float64, device=dev)
    actions_rec = torch.full((n, max_moves), 0xFF, dtype=torch.uint8, device=dev)
    probs = torch.empty((n, 4), dtype=torch.float32, device=dev)
    bits = torch.tensor([1, 2, 4, 8], dtype=torch.uint8, device=dev)
    for t in range(max_moves):
        if t % check_every == 0 and not bool(alive.any()):
            break
        if act is not None:
            actions = act(env.boards, t)
        elif mode == "greedy":
            forward(env.boards, probs)
            valid = (ops.valid_moves(env.boards)[:, None] & bits) != 0
            valid |= ~valid.any(dim=1, keepdim=True)               # no valid move: all four, as the sampler does
            actions = probs.masked_fill(~valid, float("-inf")).argmax(dim=1).to(torch.uint8)
        else:
            forward(env.boards, probs)
            mask = ops.valid_moves(env.boards) if mode == "masked" else None
            actions, _ = ops.sample_actions(probs, mask, seed, t, game_id_base)
        live = alive.bool()
        actions_rec[:, t] = torch.where(live, actions, torch.full_like(actions, 0xFF))
        _, reward, flags = ops.step(env.boards, actions, env.scores, seed, t, game_id_base, out=env.boards, reward_f64=True)
        reward_sum = torch.where(live, reward_sum + reward, reward_sum)
        ops.track_episodes(flags, alive, moves, valid_cnt, invalid_cnt, ms_move, t)
    return {"moves": moves, "valid_moves": valid_cnt, "invalid_moves": invalid_cnt, "milestone_move": ms_move, "alive": alive,
            "reward_sum": reward_sum, "actions": actions_rec}


def _select_games(results, which):
    n = len(results["scores"])
    if isinstance(which, str):
        if which == "best5":
            return list(results["best_games"])
        if which == "high_tile":                        # evaluate_beam_search.py:170: game_result['highest_tile'] >= 2048
            return [i for i, t in enumerate(results["highest_tiles"]) if t >= 2048]
        if which == "all":
            return list(range(n))
        raise ValueError("histories must be 'best5', 'high_tile', 'all' or an iterable of game indices")
    sel = [int(i) for i in which]
    if any(i < 0 or i >= n for i in sel):
        raise ValueError("histories: game index out of range")
    return sel


def game_histories(results, which, boards0, actions, moves, seed, game_id_base=0):
    """{game index: the dict evaluate_beam_search.run_game returns (evaluate_beam_search.py:86-97)} for the selected games,
    rebuilt on the device from their action bytes. boards0: the start boards of ALL games (uint8 (n,16)), actions: uint8
    (n, max_moves) as ops.play_games(want_actions=True) returned it, moves: int32 (n,)."""
    sel = _select_games(results, which)
    if not sel:
        return {}
    dev = boards0.device
    idx = torch.tensor(sel, dtype=torch.int64, device=dev)
    longest = int(moves.index_select(0, idx).max().item())
    bh, shist, fh = ops.replay_games(boards0.index_select(0, idx).contiguous(),
                                     actions.index_select(0, idx)[:, :max(longest, 1)].contiguous(),
                                     moves.index_select(0, idx).contiguous(), seed, game_ids=idx + int(game_id_base), longest=longest)
    k, hist = bh.shape[0], bh.shape[1]
    tiles = ops.unpack(bh.view(k * hist, 16)).view(k, hist, 4, 4).cpu().numpy()
    shist, fh = shist.cpu().numpy(), fh.cpu().numpy()
    acts = actions.index_select(0, idx)[:, :max(longest, 1)].cpu().numpy()
    out = {}
    for row, g in enumerate(sel):
        m = results["moves"][g]
        boards = tiles[row, :m + 1]
        ms = {t: None for t in MILESTONES}
        for t, v in results["milestones_by_game"][g].items():
            ms[t] = v
        out[g] = {
            "score": results["scores"][g], "highest_tile": results["highest_tiles"][g], "moves": m,
            "valid_moves": results["valid_moves"][g], "invalid_moves": results["invalid_moves"][g],
            "milestones": ms,
            "board_history": [b.copy() for b in boards],                       # :45 + :73: start, then the state after every move
            "max_tiles_history": [int(b.max()) for b in boards],               # :48 + :74
            "scores_history": [int(x) for x in shist[row, :m + 1]],            # :49 + :75 (starts at 0)
            "final_board": boards[m].copy(),
            "moveset": [int(a) for a in acts[row, :m]],                        # train.py:51,67
            "valid_history": [bool(f & L.FLAG_VALID) for f in fh[row, :m]],
        }
    return out


def save_moveset(game, path):
    """train.py:140-142: the move-set of one game (`results["games"][i]`, or any list of actions) as the reference writes
    `*_best_moveset_tile_N.txt` -- the actions joined by commas, no newline."""
    moveset = game["moveset"] if isinstance(game, dict) else game
    with open(path, "w") as f:
        f.write(",".join(map(str, moveset)))
    return path


def save_game_data(game, path):
    """evaluate_beam_search.py:185-196: game_{i}_data.json of one game -- the run_game dict with arrays as lists."""
    import numpy as np
    keys = ("score", "highest_tile", "moves", "valid_moves", "invalid_moves", "milestones", "board_history",
            "max_tiles_history", "scores_history", "final_board")
    out = {k: (game[k].tolist() if isinstance(game[k], np.ndarray) else game[k]) for k in keys}
    out["board_history"] = [b.tolist() if isinstance(b, np.ndarray) else b for b in game["board_history"]]
    out["milestones"] = {str(k): v for k, v in game["milestones"].items()}        # (json.dump turns the int keys into these strings)
    with open(path, "w") as f:
        json.dump(out, f)
    return path


TABLE_COLUMNS = 6 + len(MILESTONES) + 16


def results_from_table(table, elapsed, beam_width, search_depth, seed, max_moves, parameters=None):
    """The result dict from the per-game table (rows in global game order; columns as built in evaluate_beam_search).
    parameters: the "parameters" entry to use instead of the beam search's (evaluate_policy)."""
    n = table.shape[0]
    scores = table[:, 0]
    final_boards = table[:, 14:30].reshape(n, 4, 4).astype("int32")
    highest = final_boards.reshape(n, 16).max(axis=1) if n else table[:, 0]
    ms_host = table[:, 6:14]
    order = sorted(range(n), key=lambda i: scores[i], reverse=True)       # stable, like the reference's top-5 update
    best = int(order[0]) if n else 0
    results = {
        "scores": [int(s) for s in scores],
        "highest_tiles": [int(h) for h in highest],
        "moves": [int(m) for m in table[:, 1]],
        "valid_moves": [int(m) for m in table[:, 2]],
        "invalid_moves": [int(m) for m in table[:, 3]],
        "milestones": {m: [int(v) for v in ms_host[:, k] if v >= 0] for k, m in enumerate(MILESTONES)},
        "milestones_by_game": [{m: int(ms_host[g, k]) for k, m in enumerate(MILESTONES) if ms_host[g, k] >= 0} for g in range(n)],
        "best_games": [int(i) for i in order[:5]],
        "final_boards": final_boards,
        "best_board": final_boards[best].copy() if n else None,
        "best_score": int(scores[best]) if n else 0,
        "best_game_idx": best,
        "unfinished": int(table[:, 4].sum()),
        "total_moves": int(table[:, 1].sum()),
        "total_expansions": int(table[:, 5].sum()),
        "elapsed_s": elapsed,
        "parameters": parameters if parameters is not None else
                      {"beam_width": beam_width, "search_depth": search_depth, "num_games": n, "seed": seed, "max_moves": max_moves},
    }
    results["summary"] = summarize(results)
    return results


def evaluate_beam_search_sharded(num_games=4096, beam_width=20, search_depth=30, seed=0x2048, max_moves=5000, device=None,
                                 game_id_base=0, **kw):
    """The evaluation over all ranks of the default process group (one process per GPU, torchrun environment): games are
    independent and every draw is keyed by the global game id, so rank r plays the contiguous range g2048.dist.shard gives
    it with no communication, and one all-gather of the per-game table (30 int64 per game) at the end gives every rank the
    result of the whole evaluation -- identical to evaluate_beam_search(num_games) on one GPU. elapsed_s = slowest rank."""
    from . import dist as gdist
    if kw.get("histories") is not None:
        raise ValueError("evaluate_beam_search_sharded gathers the per-game table only; replay histories per rank with evaluate_beam_search")
    w, r, lr = gdist.world()
    dev = torch.device(device) if device is not None else torch.device("cuda", lr)
    lo, hi = gdist.shard(num_games, r, w)
    t0 = time.perf_counter()
    part = evaluate_beam_search(hi - lo, beam_width, search_depth, seed=seed, max_moves=max_moves, device=dev,
                                game_id_base=game_id_base + lo, _table_only=True, **kw)
    table = gdist.all_gather_rows(torch.from_numpy(part).to(dev))
    elapsed = gdist.max_over_ranks(time.perf_counter() - t0, dev)
    res = results_from_table(table.cpu().numpy(), elapsed, beam_width, search_depth, seed, max_moves)
    res["parameters"]["world_size"] = w
    return res


def summarize(results):
    """The numbers the reference prints / reports (run_evaluation.py:110-128, report.md)."""
    n = max(len(results["scores"]), 1)
    tiles = results["highest_tiles"]
    dist = {}
    for tile in tiles:
        dist[tile] = dist.get(tile, 0) + 1
    out = {
        "games": len(results["scores"]),
        "highest_tile": max(tiles) if tiles else 0,
        "best_score": max(results["scores"]) if tiles else 0,
        "average_score": sum(results["scores"]) / n,
        "average_highest_tile": sum(tiles) / n,
        "rate_2048_or_more": sum(1 for x in tiles if x >= 2048) / n,
        "tile_distribution_pct": {int(k): 100.0 * v / n for k, v in sorted(dist.items())},
        "hit_move_cap": results.get("unfinished", 0),
        "moves_per_s": results["total_moves"] / results["elapsed_s"] if results.get("elapsed_s") else None,
        "expansions_per_s": results["total_expansions"] / results["elapsed_s"] if results.get("elapsed_s") else None,
    }
    if "episode_rewards" in results:          # evaluate_policy: train.py's episode_reward
        out["average_episode_reward"] = sum(results["episode_rewards"]) / n
        out["games_per_s"] = len(results["scores"]) / results["elapsed_s"] if results.get("elapsed_s") else None
    return out


def save_overall_results(results, path):
    """overall_results.json with the reference's keys (evaluate_beam_search.py:198-214)."""
    p = results["parameters"]
    out = {
        "scores": results["scores"], "highest_tiles": results["highest_tiles"], "moves": results["moves"],
        "valid_moves": results["valid_moves"], "invalid_moves": results["invalid_moves"],
        "milestones": {str(k): v for k, v in results["milestones"].items()},
        "best_games": results["best_games"],
        "parameters": ({"beam_width": p["beam_width"], "search_depth": p["search_depth"], "num_games": p["num_games"]}
                       if "beam_width" in p else dict(p)),
    }
    if "episode_rewards" in results:          # evaluate_policy
        out["episode_rewards"] = results["episode_rewards"]
    with open(path, "w") as f:
        json.dump(out, f, indent=4)
    return path
