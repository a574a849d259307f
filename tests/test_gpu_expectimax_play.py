"""Complete games of the expectimax agent in one launch (g2048_play_expectimax_games, ops.play_expectimax_games,
g2048.evaluate_expectimax) against the move-by-move loop of expectimax_actions, step and track_episodes; against the oracle's env
step with the CPU restatement's decisions; the game-slot core's edges (a game that ends at once, unfinished games, ids that do
not start at 0, one wavefront for all games, canaries); and the drop-in agent."""
import numpy as np
import pytest
import torch

import expectimax_ref as R
import play_harness as H
from play_harness import DEV, g2048  # noqa: F401

pytestmark = pytest.mark.gpu

# full, LEFT and RIGHT alone merge the last row's pair, and whichever tile spawns in the one empty cell, no pair is left
ONE_MOVE_FROM_THE_END = [5, 3, 5, 3, 3, 5, 3, 5, 5, 3, 5, 3, 7, 8, 6, 6]


def play(n, depth, max_moves, seed, base=0, fused=True, units=0, first=None):
    """n fresh games of `seed` under the ids base + i (game 0 from the board `first`, if given), played by the one launch or by
    the move-by-move loop: the per-game dict plus the final boards and scores and the boards the games started from."""
    from g2048 import ops
    from g2048.evaluate import _play_policy_stepwise
    from g2048.vec import VecGame2048
    env = VecGame2048(n, device=torch.device(DEV), seed=seed, id_base=base)
    if first is not None:
        env.boards[0] = torch.tensor(first, dtype=torch.uint8, device=DEV)
    start = env.boards.clone()
    if fused:
        r = ops.play_expectimax_games(env.boards, env.scores, depth, max_moves, seed=seed, game_id_base=base, want_rewards=True,
                                      want_actions=True, max_waves=units)
    else:
        r = _play_policy_stepwise(env, None, None, max_moves, None, seed, base, act=lambda boards, t: ops.expectimax_actions(boards, depth))
    torch.cuda.synchronize()
    r.update(boards=env.boards, scores=env.scores, start=start)
    return r


@pytest.mark.parametrize("games,depth,max_moves", [(1, 1, 64), (65, 1, 300), (130, 2, 120)])
def test_one_launch_equals_the_move_by_move_loop(g2048, games, depth, max_moves):  # noqa: F811
    seed = 0x2048
    fused, loop = play(games, depth, max_moves, seed), play(games, depth, max_moves, seed, fused=False)
    H.assert_same(fused, loop, "one launch against the loop")
    H.check_game_invariants(fused, max_moves)
    res = g2048.evaluate_expectimax(num_games=games, depth=depth, max_moves=max_moves, seed=seed, fused=True)
    ref = g2048.evaluate_expectimax(num_games=games, depth=depth, max_moves=max_moves, seed=seed, fused=False)
    for k in H.RESULT_KEYS:
        assert res[k] == ref[k], k
    assert set(res) == set(ref)
    assert np.array_equal(res["final_boards"], ref["final_boards"]) and np.array_equal(res["best_board"], ref["best_board"])
    assert res["parameters"] == {"depth": depth, "early_game_threshold": 512, "mid_game_threshold": 1024, "max_moves": max_moves,
                                 "num_games": games, "seed": seed}
    assert res["scores"] == fused["scores"].cpu().tolist() and res["moves"] == fused["moves"].cpu().tolist()
    assert res["unfinished"] == int(fused["alive"].sum()) > 0, "max_moves is small enough that games stay unfinished"


def test_a_game_one_move_from_its_end_and_ids_that_do_not_start_at_0(g2048, oracle):  # noqa: F811
    first = np.array([ONE_MOVE_FROM_THE_END], np.uint8)
    assert oracle.valid_moves_batch(first)[0] == 0b0101 and (first != 0).all()
    seed, base, cap = 11, 1000003, 48
    fused = play(9, 1, cap, seed, base, first=ONE_MOVE_FROM_THE_END)
    loop = play(9, 1, cap, seed, base, fused=False, first=ONE_MOVE_FROM_THE_END)
    H.assert_same(fused, loop, "a game that ends at once, ids from %d" % base)
    H.check_game_invariants(fused, cap)
    assert int(fused["moves"][0]) == 1 and int(fused["alive"][0]) == 0 and int(fused["valid_moves"][0]) == 1
    assert int(fused["actions"][0, 0]) == int(R.decide(first, 1)[0][0]) and bool((fused["actions"][0, 1:] == 0xFF).all())
    assert int(fused["alive"][1:].sum()) == 8, "the fresh games outlast the cap"
    # the games belong to their ids, not to the launch: ids base + 3 .. base + 8 played apart are games 3 .. 8
    apart = play(6, 1, cap, seed, base + 3)
    for k in H.KEYS:
        assert torch.equal(apart[k], fused[k][3:]), k
    assert not torch.equal(play(9, 1, cap, seed, 0)["boards"][1:], fused["boards"][1:]), "the ids do not reach the draws"


def test_one_wavefront_plays_every_game_and_two_launches_agree(g2048):  # noqa: F811
    """A unit cap of 1: every game after the first comes from the ticket counter, one after another on the same wavefront."""
    seed, cap = 5, 40
    whole = play(7, 1, cap, seed)
    for units in (1, 2, 3):
        H.assert_same(whole, play(7, 1, cap, seed, units=units), "max_waves=%d" % units)
    H.assert_same(whole, play(7, 1, cap, seed), "two launches")
    deep = play(3, 2, 12, seed)
    H.assert_same(deep, play(3, 2, 12, seed, units=1), "depth 2, max_waves=1")
    # depth 3 on fresh boards (thirteen and more empty cells: the widest trees there are), three moves of two games
    H.assert_same(play(2, 3, 3, seed), play(2, 3, 3, seed, fused=False), "depth 3 against the loop")


@pytest.mark.parametrize("depth,games,cap", [(1, 6, 40), (2, 2, 8)])
def test_recorded_actions_replay_through_the_oracle(g2048, oracle, depth, games, cap):  # noqa: F811
    """The oracle's env step on the recorded actions reproduces every intermediate and final board, score, counter, milestone and
    f64 reward sum, and every recorded action is the CPU restatement's decision for the board it was taken on."""
    seed = 21
    r = play(games, depth, cap, seed)
    bh, sh, _, _ = H.replay(None, None, r, seed, want_outputs=False)

    def expected(t, boards, mask, live):
        want = np.zeros(len(boards), np.uint8)
        want[live] = R.decide(boards[live], depth)[0]
        return (want,)

    H.check_games_against_oracle(oracle, r, (bh, sh), seed, expected)


def test_canaries_and_one_move(g2048):  # noqa: F811
    """The C entry point called raw on n of n + 37 rows: nothing is written past n, and the first n rows are the wrapper's."""
    from g2048 import _lib as L
    from g2048.vec import VecGame2048
    dev, extra, seed = torch.device(DEV), 37, 3
    lib = L.search_lib()
    for n, cap in ((3, 1), (66, 20)):
        env = VecGame2048(n + extra, device=dev, seed=seed)
        boards, scores = env.boards.clone(), env.scores.clone()
        outs = {"moves": torch.full((n + extra,), -7, dtype=torch.int32, device=DEV),
                "valid_moves": torch.full((n + extra,), -7, dtype=torch.int32, device=DEV),
                "invalid_moves": torch.full((n + extra,), -7, dtype=torch.int32, device=DEV),
                "milestone_move": torch.full((n + extra, 8), -7, dtype=torch.int32, device=DEV),
                "reward_sum": torch.full((n + extra,), -7.0, dtype=torch.float64, device=DEV),
                "alive": torch.full((n + extra,), 7, dtype=torch.uint8, device=DEV),
                "actions": torch.full((n + extra, cap), 7, dtype=torch.uint8, device=DEV)}
        nb = lib.g2048_play_expectimax_workspace(n)
        ws = torch.full((nb + 64,), 0x5A, dtype=torch.uint8, device=DEV)
        L.search_call(dev, lib.g2048_play_expectimax_games, boards.data_ptr(), scores.data_ptr(), 1, 512, 1024,
                      *(v.data_ptr() for v in outs.values()), cap, seed, 0, n, 0, ws.data_ptr(), nb, L.stream_ptr(dev))
        torch.cuda.synchronize()
        assert torch.equal(boards[n:], env.boards[n:]) and torch.equal(scores[n:], env.scores[n:])
        assert bool((ws[nb:] == 0x5A).all()), "written past the workspace"
        for k, v in outs.items():
            assert bool((v[n:] == (7 if k in ("alive", "actions") else -7)).all()), "%s written past n = %d" % (k, n)
        ref = play(n, 1, cap, seed)
        assert torch.equal(boards[:n], ref["boards"]) and torch.equal(scores[:n], ref["scores"])
        for k, v in outs.items():
            assert torch.equal(v[:n], ref[k]), "n = %d, cap = %d: %s is not the wrapper's" % (n, cap, k)
        if cap == 1:
            assert bool((outs["moves"][:n] == 1).all()) and bool((outs["alive"][:n] == 1).all())


def test_drop_in_agent_plays_the_batched_decisions(g2048):  # noqa: F811
    """20 moves of ExpectimaxAgent(depth=1) on the drop-in Game2048Env, a train.py-shaped loop: every action is what the batched
    call answers for the same board, with and without the env's valid moves handed in."""
    from agents.expectimax_agent import ExpectimaxAgent
    from environment.game_2048 import Game2048Env
    from g2048 import ops
    env, agent = Game2048Env(seed=77), ExpectimaxAgent(depth=1)
    state = env.reset()
    seen, taken = [], []
    for t in range(20):
        valid = env.get_valid_moves()
        action, log_prob = agent.get_action(state, valid if t % 2 else None)
        assert log_prob == 0.0 and valid[action]
        seen.append(np.asarray(state, dtype=np.int32).reshape(16))
        taken.append(action)
        next_state, reward, done, info = env.step(action)
        agent.remember(state, action, reward, next_state, done, log_prob)
        state = next_state
        assert not done
    agent.update()
    codes = ops.pack(torch.as_tensor(np.stack(seen), device=DEV))
    batched = g2048.BatchedExpectimax(depth=1).get_actions(codes)
    assert batched.cpu().tolist() == taken
    assert R.decide(codes.cpu().numpy(), 1)[0].tolist() == taken
