"""What the GPU tests of the four "complete games in one launch" kernels have in common (tests/test_gpu_policy_play.py,
test_gpu_tpolicy_play.py, test_gpu_qnet_play.py, test_gpu_qnet_beam.py): the module fixture, one `play`, and one copy of each
check, so that the one device core (csrc/g2048_play.h) is held to one standard. A `Kernel` says what differs between the four;
the test files keep their networks, shapes, seeds and bounds.

`how` is what a kernel takes besides the network: the mode of the two policies, epsilon of the Q-network, (epsilon, beam_width,
search_depth, threshold) of the Q-network with its search. A bare value stands for the one-element tuple."""
from collections import namedtuple

import numpy as np
import pytest
import torch

DEV = "cuda:0"
KEYS = ("boards", "scores", "moves", "valid_moves", "invalid_moves", "milestone_move", "alive", "reward_sum", "actions")
RESULT_KEYS = ("scores", "highest_tiles", "moves", "valid_moves", "invalid_moves", "milestones", "milestones_by_game", "best_games",
               "best_score", "best_game_idx", "unfinished", "total_moves", "total_expansions", "episode_rewards", "parameters")


@pytest.fixture(scope="module")
def g2048():
    import __graft_entry__ as ge
    ge.ensure_built()
    return ge.import_package()


# entry:     ops.play_<entry>_games, g2048_play_<entry>_games and g2048_play_<entry>_workspace
# units:     the name of the wrapper's unit cap
# net_args:  net -> the network arguments of the wrapper (the blob first); the C entry point takes the blob's address
# stepwise:  (net, n, how, seed, base) -> (mode, keyword arguments) of evaluate._play_policy_stepwise, the unfused yardstick
# raw_how:   how -> (the C entry point's arguments between max_moves and seed, bits to OR into its opts)
# forward:   (net, boards) -> the device forward's float32 (n, 4) on replayed boards
Kernel = namedtuple("Kernel", "entry units net_args stepwise raw_how forward")


def _encoder_args(net):
    return net.packed, net.dim_ff, net.n_layers


def _mode_bits(how):
    from g2048 import _lib as L
    from g2048 import ops
    return (), ops.PLAY_POLICY_MODES[how[0]] << L.PLAY_POLICY_MODE_SHIFT


def _policy_forward(net, boards):
    from g2048 import ops
    return ops.policy_forward(boards, net.actor.blob(1), None, net.precision)


def _tpolicy_forward(net, boards, probs=None):
    from g2048 import ops
    return ops.tpolicy_forward(boards, net.packed, net.dim_ff, net.n_layers, net.precision, probs=probs, want_value=False)


def _qnet_forward(net, boards):
    from g2048 import ops
    return ops.qnet_forward(boards, net.packed, net.dim_ff, net.n_layers, net.precision)


def _qnet_stepwise(net, n, how, seed, base):
    from g2048.evaluate import qnet_stepwise_act
    return None, {"act": qnet_stepwise_act(net.packed, net.dim_ff, net.n_layers, net.precision, n, torch.device(DEV), how[0], seed, base,
                                           how[1:] or None)}


POLICY = Kernel("policy", "max_waves", lambda net: (net.actor.blob(1),), lambda net, n, how, seed, base: (how[0], {}), _mode_bits,
                _policy_forward)
TPOLICY = Kernel("tpolicy", "max_blocks", _encoder_args,
                 lambda net, n, how, seed, base: (how[0], {"forward": lambda boards, probs: _tpolicy_forward(net, boards, probs)}),
                 _mode_bits, _tpolicy_forward)
QNET = Kernel("qnet", "max_waves", _encoder_args, _qnet_stepwise, lambda how: (how, 0), _qnet_forward)
QNET_BEAM = QNET._replace(entry="qnet_beam")            # the same network and yardstick; `how` carries the beam's settings


def _tuple(how):
    return how if isinstance(how, tuple) else (how,)


def play(kernel, net, n, max_moves, how, seed, base=0, fused=True, units=0):
    """n fresh games of `seed` under the ids base + i, played by the one launch or by the unfused loop: the wrapper's result
    dict plus the final boards and scores and the boards the games started from."""
    from g2048 import ops
    from g2048.evaluate import _play_policy_stepwise
    from g2048.vec import VecGame2048
    how = _tuple(how)
    env = VecGame2048(n, device=torch.device(DEV), seed=seed, id_base=base)
    start = env.boards.clone()
    net_args = kernel.net_args(net)
    if fused:
        r = getattr(ops, "play_%s_games" % kernel.entry)(env.boards, env.scores, *net_args, net.precision, max_moves, *how, seed, base,
                                                         want_rewards=True, want_actions=True, **{kernel.units: units})
    else:
        mode, kw = kernel.stepwise(net, n, how, seed, base)
        r = _play_policy_stepwise(env, net_args[0], net.precision, max_moves, mode, seed, base, **kw)
    torch.cuda.synchronize()
    r.update(boards=env.boards, scores=env.scores, start=start)
    return r


def assert_same(a, b, what):
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), "%s: %s differ" % (what, k)


def check_game_invariants(r, cap):
    if cap == 37:
        assert int(r["alive"].sum()) > 0 and int((r["moves"] == 37).sum()) >= int(r["alive"].sum())
    assert int(r["moves"].min()) >= 1 and bool((r["valid_moves"] + r["invalid_moves"] == r["moves"]).all())
    assert bool((r["moves"] <= cap).all()) and bool(((r["moves"] == cap) | (r["alive"] == 0)).all())


def replay(kernel, net, r, seed, want_outputs):
    """Every pre-move board of every game (g2048_replay_games) and, if asked, the device forward's output for it (exact, because
    the forward does not depend on placement): board histories, score histories, outputs (k, longest, 4) or None, longest."""
    from g2048 import ops
    longest = int(r["moves"].max().item())
    bh, sh, _ = ops.replay_games(r["start"], r["actions"], r["moves"], seed, longest=longest)
    k = bh.shape[0]
    out = None
    if want_outputs:
        out = kernel.forward(net, bh[:, :longest].reshape(k * longest, 16).contiguous()).view(k, longest, 4).cpu().numpy()
    torch.cuda.synchronize()
    return bh.cpu().numpy(), sh.cpu().numpy(), out, longest


def check_games_against_oracle(oracle, r, histories, seed, expected_actions):
    """Replaying the recorded actions with the oracle's env step gives g2048_replay_games' histories (bh, sh) and the kernel's
    final state, counters, milestones and f64 reward sums, and every recorded action is the expected one.
    expected_actions(t, boards, mask, live) -> (actions (n,), ...) for move t of all n games, mask = the oracle's valid moves.
    Returns per move (live, whatever expected_actions returned after the actions)."""
    bh, sh = histories
    moves = r["moves"].cpu().numpy()
    acts = r["actions"].cpu().numpy()
    n, longest = len(moves), int(moves.max())
    b = r["start"].cpu().numpy()
    sc = np.zeros(n, np.uint32)
    rsum = np.zeros(n, np.float64)
    ms = np.full((n, 8), -1, np.int64)
    valid = np.zeros(n, np.int64)
    notes = []
    for t in range(longest):
        live = t < moves
        assert np.array_equal(b[live], bh[live, t]) and np.array_equal(sc[live], sh[live, t].astype(np.uint32))
        want, *rest = expected_actions(t, b, oracle.valid_moves_batch(b), live)
        assert np.array_equal(want[live], acts[live, t]), "move %d: the recorded actions are not the expected ones" % t
        notes.append((live, rest))
        a = np.where(live, acts[:, t], 0).astype(np.uint8)
        nb, nsc, rw, fl = oracle.step_batch(b, a, sc, seed, t, 0)
        b = np.where(live[:, None], nb, b)
        sc = np.where(live, nsc, sc)
        rsum = np.where(live, rsum + rw, rsum)
        valid += (live & ((fl & 2) != 0)).astype(np.int64)
        code = (fl >> 3).astype(np.int64)
        for k in range(8):
            ms[:, k] = np.where(live & (ms[:, k] < 0) & (code >= 6 + k), t, ms[:, k])
    fin = np.arange(n)
    assert np.array_equal(b, bh[fin, moves]) and np.array_equal(sc, sh[fin, moves].astype(np.uint32))
    assert np.array_equal(b, r["boards"].cpu().numpy()) and np.array_equal(sc, r["scores"].cpu().numpy().astype(np.uint32))
    assert np.array_equal(rsum, r["reward_sum"].cpu().numpy()), "f64 reward sums differ"
    assert np.array_equal(valid, r["valid_moves"].cpu().numpy()) and np.array_equal(ms, r["milestone_move"].cpu().numpy())
    assert np.array_equal(moves - valid, r["invalid_moves"].cpu().numpy())
    assert bool((acts[np.arange(acts.shape[1])[None, :] >= moves[:, None]] == 0xFF).all())
    return notes


def check_decisions_against_f64(oracle, r, bh, seed, masked, probs_f64, gap_bound, rate_bound=None, what=""):
    """Every recorded decision against the oracle's sampling from f64 probabilities, probs_f64(boards uint8 (k,16)) -> (k,4): a
    different decision is allowed only where the draw lies within gap_bound (relative to the CDF total) of a CDF boundary,
    and, with a rate_bound, at most that share of all decisions may differ."""
    moves = r["moves"].cpu().numpy()
    acts = r["actions"].cpu().numpy()
    game, move = np.nonzero(np.arange(int(moves.max()))[None, :] < moves[:, None])          # every decision (game, move)
    boards = bh[game, move]
    p64 = probs_f64(boards)
    mask = oracle.valid_moves_batch(boards) if masked else np.full(len(game), 15, np.uint8)
    keys = [oracle.rng_keys(seed, oracle.DOM_POLICY, t) for t in range(int(moves.max()))]
    u = np.array([oracle.rng_draw(keys[t][0], keys[t][1], int(i), 0) >> 8 for i, t in zip(game, move)], np.float64) * 2.0 ** -24
    m = np.where(mask == 0, 15, mask)
    w = np.where((m[:, None] >> np.arange(4)) & 1, p64 + 1e-10, 0.0)
    cdf = np.cumsum(w, axis=1)
    x = u * cdf[:, 3]
    want = (x[:, None] >= cdf[:, :3]).sum(axis=1)
    top = np.array([int(v).bit_length() - 1 for v in m])              # rounding past the last valid action (sample_action)
    want = np.where((m >> want) & 1, want, top)
    bad = want != acts[game, move]
    gap = np.abs(cdf[bad, :3] - x[bad, None]).min(axis=1) / cdf[bad, 3]
    print("%s: %d decisions, %d differ from the f64 forward (%.3g of all; largest gap to a CDF boundary %.3g, bound %g)" % (
        what, len(game), int(bad.sum()), bad.mean(), gap.max() if bad.any() else 0.0, gap_bound))
    assert (gap <= gap_bound).all(), "decisions differ away from a CDF boundary (gap %.3g)" % gap.max()
    if rate_bound is not None:
        assert bad.sum() <= rate_bound * len(game)


def check_canaries(kernel, net, how, shapes):
    """The C entry point called raw on n of n + 37 rows, per (n, cap) of shapes: nothing is written past n, and the first n rows
    are the wrapper's result. Seed 3, ids from 0, as many units as the chip holds."""
    from g2048 import _lib as L
    from g2048.vec import VecGame2048
    dev, extra, seed = torch.device(DEV), 37, 3
    pre, opt_bits = kernel.raw_how(_tuple(how))
    opts = (L.POLICY_BF16 if net.precision == "bf16" else L.POLICY_F32) | opt_bits
    net_args = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in kernel.net_args(net)]
    for n, cap in shapes:
        env = VecGame2048(n + extra, device=dev, seed=seed)
        boards, scores = env.boards.clone(), env.scores.clone()
        outs = {"moves": torch.full((n + extra,), -7, dtype=torch.int32, device=DEV),
                "valid_moves": torch.full((n + extra,), -7, dtype=torch.int32, device=DEV),
                "invalid_moves": torch.full((n + extra,), -7, dtype=torch.int32, device=DEV),
                "milestone_move": torch.full((n + extra, 8), -7, dtype=torch.int32, device=DEV),
                "reward_sum": torch.full((n + extra,), -7.0, dtype=torch.float64, device=DEV),
                "alive": torch.full((n + extra,), 7, dtype=torch.uint8, device=DEV),
                "actions": torch.full((n + extra, cap), 7, dtype=torch.uint8, device=DEV)}
        ws = torch.empty(getattr(L.lib(), "g2048_play_%s_workspace" % kernel.entry)(n), dtype=torch.uint8, device=DEV)
        L.call(dev, getattr(L.lib(), "g2048_play_%s_games" % kernel.entry), boards.data_ptr(), scores.data_ptr(), *net_args,
               *(v.data_ptr() for v in outs.values()), cap, *pre, seed, 0, n, opts, 0, ws.data_ptr(), ws.numel(), L.stream_ptr(dev))
        torch.cuda.synchronize()
        assert torch.equal(boards[n:], env.boards[n:]) and torch.equal(scores[n:], env.scores[n:])
        for k, v in outs.items():
            assert bool((v[n:] == (7 if k in ("alive", "actions") else -7)).all()), "%s written past n = %d" % (k, n)
        ref = play(kernel, net, n, cap, how, seed)
        assert torch.equal(boards[:n], ref["boards"]) and torch.equal(scores[:n], ref["scores"])
        for k, v in outs.items():
            assert torch.equal(v[:n], ref[k]), "n = %d, cap = %d: %s is not the wrapper's" % (n, cap, k)
        if cap == 1:
            assert bool((outs["moves"][:n] == 1).all()) and bool((outs["alive"][:n] == 1).all())


def check_independence(kernel, net, n, max_moves, how, seed, base, units=(), split=None, what=""):
    """The games do not depend on the number of units that play them, nor, with `split`, on the launch (a second one gives the
    same) or on which launch plays an id (the first `split` ids and the rest, played apart). Returns the games."""
    whole = play(kernel, net, n, max_moves, how, seed, base=base)
    for u in units:
        assert_same(whole, play(kernel, net, n, max_moves, how, seed, base=base, units=u), "%s %s=%d" % (what, kernel.units, u))
    if split is not None:
        assert_same(whole, play(kernel, net, n, max_moves, how, seed, base=base), "two launches")
        lo = play(kernel, net, split, max_moves, how, seed, base=base)
        hi = play(kernel, net, n - split, max_moves, how, seed, base=base + split)
        for k in KEYS:
            assert torch.equal(torch.cat([lo[k], hi[k]]), whole[k]), "split at %d: %s differs" % (split, k)
    return whole


def check_evaluate_drivers(evaluate_fn, net, kw, expected_parameters):
    """evaluate_fn(net, **kw) with the one launch against fused=False, and the histories of its best five games. Returns the
    fused results."""
    res = evaluate_fn(net, histories="best5", **kw)
    ref = evaluate_fn(net, fused=False, **kw)
    for k in RESULT_KEYS:
        assert res[k] == ref[k], k
    assert set(res) - {"games"} == set(ref)
    assert np.array_equal(res["final_boards"], ref["final_boards"]) and np.array_equal(res["best_board"], ref["best_board"])
    assert res["parameters"] == expected_parameters
    assert sorted(res["games"]) == sorted(res["best_games"])
    for i, game in res["games"].items():
        assert np.array_equal(game["board_history"][-1], res["final_boards"][i])
        assert game["scores_history"][-1] == res["scores"][i] and len(game["moveset"]) == res["moves"][i]
    print(res["summary"])
    return res
