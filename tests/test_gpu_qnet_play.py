"""g2048_qnet_select_actions and g2048_play_qnet_games on the MI355X: the select launch against a NumPy restatement of
DQNAgent.select_action, the fused kernel against the unfused loop of the launches that exist apart from it (every output, bit
for bit), the recorded games against the CPU oracle and the recorded decisions against the NumPy select_action on the device
forward's own Q, the greedy decisions against qnet.forward_reference in float64, independence of the wavefront count and of
the id split, canaries past n, and evaluate_qnet.

The networks carry the hash-derived weights of tests/qnet_weights.py: the fixture's (dim_ff 2048, 2 layers) and a small one
(dim_ff 32, 1 layer)."""
import numpy as np
import pytest
import torch

import qnet_weights as qw
from test_gpu_qnet import LEFT_OUT_CAP, module_rows_f32, q_bound
from test_policy_host import random_boards
from test_qnet_host import RefSpelling, bf16_round, golden_model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("boards", "scores", "moves", "valid_moves", "invalid_moves", "milestone_move", "alive", "reward_sum", "actions")
_MODELS, _NETS = {}, {}

DEAD = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1]                 # full, no merge: no valid move
ONLY_RIGHT = [1, 2, 1, 0, 2, 1, 2, 0, 1, 2, 1, 0, 2, 1, 2, 0]
ONLY_DOWN = [3, 4, 3, 4, 4, 3, 4, 3, 3, 4, 3, 4, 0, 0, 0, 0]
BIASED_LEFT_UP = [0, 0, 0, 0, 0, 0, 1, 2, 0, 1, 2, 3, 0, 2, 3, 7]       # 128 in the corner; neither RIGHT nor DOWN moves anything
BIASED_LEFT_RIGHT = [1, 1, 2, 3, 2, 3, 1, 2, 1, 2, 3, 1, 2, 1, 2, 8]    # 256 in the corner; full, one horizontal pair


@pytest.fixture(scope="module")
def g2048():
    import __graft_entry__ as ge
    ge.ensure_built()
    return ge.import_package()


def hash_model(network):
    """RefSpelling in float64 eval mode, on the CPU, carrying the hash-derived weights: the fixture's network or the small one."""
    if network not in _MODELS:
        if network == "fixture":
            model = golden_model()[2]
        else:
            model = RefSpelling(32, 1).double()
            shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
            assert shapes == qw.reference_shapes(32, 1)
            model.load_state_dict({k: torch.from_numpy(v) for k, v in qw.state_dict(shapes).items()})
            model = model.eval()
        _MODELS[network] = model
    return _MODELS[network]


def device_net(network, precision):
    key = (network, precision)
    if key not in _NETS:
        import copy
        from g2048 import DeviceQNetwork
        _NETS[key] = DeviceQNetwork(copy.deepcopy(hash_model(network)).float().to(DEV), precision=precision)
    return _NETS[key]


def play(net, n, max_moves, epsilon, seed, base=0, fused=True, max_waves=0):
    from g2048 import ops
    from g2048.evaluate import _play_policy_stepwise, qnet_stepwise_act
    from g2048.vec import VecGame2048
    env = VecGame2048(n, device=torch.device(DEV), seed=seed, id_base=base)
    start = env.boards.clone()
    if fused:
        r = ops.play_qnet_games(env.boards, env.scores, net.packed, net.dim_ff, net.n_layers, net.precision, max_moves, epsilon, seed,
                                base, want_rewards=True, want_actions=True, max_waves=max_waves)
    else:
        act = qnet_stepwise_act(net.packed, net.dim_ff, net.n_layers, net.precision, n, torch.device(DEV), epsilon, seed, base)
        r = _play_policy_stepwise(env, net.packed, net.precision, max_moves, None, seed, base, act=act)
    torch.cuda.synchronize()
    r.update(boards=env.boards, scores=env.scores, start=start)
    return r


def assert_same(a, b, what):
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), "%s: %s differ" % (what, k)


def biased_boards(boards):
    """hybrid.py:922-927 on uint8 codes: max tile >= 64 and np.argmax(board) == (3, 3) (the FIRST maximum is the corner)."""
    b = np.asarray(boards)
    return (b.max(axis=1) >= 6) & (np.argmax(b, axis=1) == 15)


def select_action_np(oracle, q, boards, mask, epsilon, seed, t, base):
    """DQNAgent.select_action (hybrid.py:909-953, use_beam_search = False) for boards with ids base + i at step t, restated with
    the oracle's draws: (actions, explored, biased)."""
    n = len(boards)
    k0, k1 = oracle.rng_keys(seed, oracle.DOM_POLICY, t)
    draws = np.array([oracle.rng_draw(k0, k1, base + i, 1) >> 8 for i in range(n)], np.uint32)
    explored = draws.astype(np.float32) * np.float32(2.0 ** -24) < np.float32(epsilon)
    biased = biased_boards(boards)
    prefs = np.where(biased[:, None], np.array([1, 1, 3, 3], np.float32) / np.float32(8), np.float32(0.25)).astype(np.float32)
    sampled, _ = oracle.sample_batch(prefs, mask, seed, t, base)
    exploit = qw.masked_argmax(q, qw.mask_bits(mask))
    return np.where(explored, sampled, exploit).astype(np.uint8), explored, biased


def test_select_launch_against_numpy(g2048, oracle):
    from g2048 import ops
    boards = np.concatenate([random_boards(4096, 9), np.array([DEAD, ONLY_RIGHT, ONLY_DOWN, BIASED_LEFT_UP, BIASED_LEFT_RIGHT], np.uint8)])
    n = len(boards)
    mask = oracle.valid_moves_batch(boards)
    assert list(mask[4096:]) == [0, 4, 8, 3, 5]
    assert list(biased_boards(boards[4096:])) == [False, False, False, True, True]
    assert biased_boards(boards).sum() >= 100 and (qw.mask_bits(mask).sum(axis=1) < 4).sum() >= 50
    net = device_net("fixture", "f32")
    b = torch.from_numpy(boards).to(DEV)
    greedy, q = [x.clone() for x in net.act(b)]
    assert torch.equal(ops.valid_moves(b).cpu(), torch.from_numpy(mask))
    qh = q.cpu().numpy()
    assert np.array_equal(greedy.cpu().numpy(), qw.masked_argmax(qh, qw.mask_bits(mask)))
    seed = 0x5EED
    for t, base in ((0, 0), (1234, (1 << 33) + 5)):
        for epsilon in (0.0, 0.25, 1.0):
            want, want_explored, biased = select_action_np(oracle, qh, boards, mask, epsilon, seed, t, base)
            actions = torch.full((n + 13,), 9, dtype=torch.uint8, device=DEV)
            explored = torch.full((n + 13,), 9, dtype=torch.uint8, device=DEV)
            ops.qnet_select_actions(q, b, epsilon, seed, t, base, actions=actions[:n], explored=explored[:n])
            torch.cuda.synchronize()
            assert bool((actions[n:] == 9).all()) and bool((explored[n:] == 9).all()), "rows past n were written"
            got, got_explored = actions[:n].cpu().numpy(), explored[:n].cpu().numpy()
            assert np.array_equal(got_explored, want_explored.astype(np.uint8)), "coins differ (epsilon %g, step %d)" % (epsilon, t)
            assert np.array_equal(got, want), "actions differ (epsilon %g, step %d)" % (epsilon, t)
            if epsilon == 0.0:
                assert not got_explored.any() and np.array_equal(got, greedy.cpu().numpy())
            if epsilon == 1.0:
                assert got_explored.all()
                ok = qw.mask_bits(np.where(mask == 0, 15, mask))
                assert ok[np.arange(n), got].all(), "an explored action is invalid"
                assert got[4097] == 2 and got[4098] == 3 and got[4099] in (0, 1) and got[4100] in (0, 2)
            print("epsilon %g step %d base %d: %d explored, %d of them with the biased preferences" % (
                epsilon, t, base, got_explored.sum(), (got_explored.astype(bool) & biased).sum()))
            a2, q2 = net.act(b, epsilon, seed, t, base)                                   # the same through DeviceQNetwork.act
            assert np.array_equal(a2.cpu().numpy(), want) and torch.equal(q2, q)
    assert torch.equal(net.act(b)[0], greedy)


@pytest.mark.parametrize("network", ["fixture", "small"])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("epsilon", [0.0, 0.25, 1.0])
def test_fused_equals_unfused(g2048, epsilon, precision, network):
    net = device_net(network, precision)
    for n, cap in ((1, 2000), (31, 2000), (33, 2000), (129, 2000), (4097, 2000), (4097, 37)):
        seed = 1000 + n + cap
        a = play(net, n, cap, epsilon, seed, fused=False)
        b = play(net, n, cap, epsilon, seed, fused=True)
        assert_same(a, b, "epsilon %g %s %s n=%d cap=%d" % (epsilon, precision, network, n, cap))
        if cap == 37:
            assert int(b["alive"].sum()) > 0 and int((b["moves"] == 37).sum()) >= int(b["alive"].sum())
        assert int(b["moves"].min()) >= 1 and bool((b["valid_moves"] + b["invalid_moves"] == b["moves"]).all())
        assert bool((b["moves"] <= cap).all()) and bool(((b["moves"] == cap) | (b["alive"] == 0)).all())
        if n == 4097 and cap == 2000:
            m = b["moves"].double()
            print("%s %s epsilon %g: mean game %.1f moves, longest %d" % (network, precision, epsilon, m.mean().item(), int(m.max().item())))


def replay(net, r, seed, want_q):
    """Every pre-move board of every game (g2048_replay_games) and, if asked, the network's Q for it (g2048_qnet_forward; exact,
    because the forward does not depend on placement)."""
    from g2048 import ops
    longest = int(r["moves"].max().item())
    bh, sh, _ = ops.replay_games(r["start"], r["actions"], r["moves"], seed, longest=longest)
    k = bh.shape[0]
    q = None
    if want_q:
        q = ops.qnet_forward(bh[:, :longest].reshape(k * longest, 16).contiguous(), net.packed, net.dim_ff, net.n_layers, net.precision)
        q = q.view(k, longest, 4).cpu().numpy()
    torch.cuda.synchronize()
    return bh.cpu().numpy(), sh.cpu().numpy(), q, longest


def test_recorded_games_against_the_oracle(g2048, oracle):
    """256 complete games at epsilon 0.25: replaying the recorded actions with the oracle's env step gives g2048_replay_games'
    histories and the kernel's final state, counters, milestones and f64 reward sums; the NumPy select_action on the device
    forward's Q of every pre-move board gives the recorded action of every move."""
    net = device_net("fixture", "f32")
    n, seed, epsilon = 256, 4242, 0.25
    r = play(net, n, 2000, epsilon, seed)
    bh, sh, q, longest = replay(net, r, seed, True)
    moves = r["moves"].cpu().numpy()
    acts = r["actions"].cpu().numpy()
    b = r["start"].cpu().numpy()
    sc = np.zeros(n, np.uint32)
    rsum = np.zeros(n, np.float64)
    ms = np.full((n, 8), -1, np.int64)
    valid = np.zeros(n, np.int64)
    explored_biased = explored_all = 0
    for t in range(longest):
        live = t < moves
        assert np.array_equal(b[live], bh[live, t]) and np.array_equal(sc[live], sh[live, t].astype(np.uint32))
        mask = oracle.valid_moves_batch(b)
        want, explored, biased = select_action_np(oracle, q[:, t], b, mask, epsilon, seed, t, 0)
        assert np.array_equal(want[live], acts[live, t]), "move %d: select_action picks different actions" % t
        explored_all += int((live & explored).sum())
        explored_biased += int((live & explored & biased).sum())
        a = np.where(live, acts[:, t], 0).astype(np.uint8)
        nb, nsc, rw, fl = oracle.step_batch(b, a, sc, seed, t, 0)
        b = np.where(live[:, None], nb, b)
        sc = np.where(live, nsc, sc)
        rsum = np.where(live, rsum + rw, rsum)
        valid += (live & ((fl & 2) != 0)).astype(np.int64)
        code = (fl >> 3).astype(np.int64)
        for k in range(8):
            ms[:, k] = np.where(live & (ms[:, k] < 0) & (code >= 6 + k), t, ms[:, k])
    print("%d decisions, %d explored, %d of them with the biased preferences" % (moves.sum(), explored_all, explored_biased))
    assert explored_biased > 0 and 0.2 * moves.sum() < explored_all < 0.3 * moves.sum()
    fin = np.arange(n)
    assert np.array_equal(b, bh[fin, moves]) and np.array_equal(sc, sh[fin, moves].astype(np.uint32))
    assert np.array_equal(b, r["boards"].cpu().numpy()) and np.array_equal(sc, r["scores"].cpu().numpy().astype(np.uint32))
    assert np.array_equal(rsum, r["reward_sum"].cpu().numpy()), "f64 reward sums differ"
    assert np.array_equal(valid, r["valid_moves"].cpu().numpy()) and np.array_equal(ms, r["milestone_move"].cpu().numpy())
    assert np.array_equal(moves - valid, r["invalid_moves"].cpu().numpy())
    assert bool((acts[np.arange(acts.shape[1])[None, :] >= moves[:, None]] == 0xFF).all())


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_greedy_decisions_against_f64(g2048, oracle, precision):
    """Every decision of 256 greedy games against the masked argmax of qnet.forward_reference in float64 on the pre-move board.
    The Q bound is tests/test_gpu_qnet.py's, taken over these boards (f32: 8 x the CPU-f32 error, bf16: 4 x the weights-only
    error); a decision may differ only where the f64 top-two gap is within twice that bound, and the share of such boards is
    capped at LEFT_OUT_CAP."""
    from g2048 import qnet
    model = hash_model("fixture")
    parsed = qnet.parse(model)
    net = device_net("fixture", precision)
    n, seed = 256, 4242
    r = play(net, n, 2000, 0.0, seed)
    bh, _, _, longest = replay(net, r, seed, False)
    moves = r["moves"].cpu().numpy()
    acts = r["actions"].cpu().numpy()
    game, move = np.nonzero(np.arange(longest)[None, :] < moves[:, None])           # every decision (game, move)
    boards = bh[game, move]
    tb = torch.from_numpy(boards)
    chunks = range(0, len(boards), 4096)
    truth = torch.cat([qnet.forward_reference(parsed, tb[i:i + 4096]) for i in chunks]).numpy()
    if precision == "f32":
        import copy
        f32_cpu, rounded = module_rows_f32(copy.deepcopy(model), boards), None
    else:
        f32_cpu, rounded = None, torch.cat([qnet.forward_reference(parsed, tb[i:i + 4096], round_weights=bf16_round) for i in chunks]).numpy()
    bound = q_bound(precision, truth, f32_cpu, rounded)
    valid = qw.mask_bits(oracle.valid_moves_batch(boards))
    gap = qw.top_two_gap(truth, valid)
    clear = gap > 2 * bound
    left_out = 1.0 - clear.mean()
    wrong = acts[game, move] != qw.masked_argmax(truth, valid)
    print("greedy %s: %d decisions, Q bound %.3g, smallest gap %.3g, %.2f %% within twice the bound of a tie (cap %.0f %%); differing "
          "decisions: %d among the clear, %d among the rest" % (precision, len(game), bound, gap.min(), 100 * left_out,
                                                                 100 * LEFT_OUT_CAP[precision], (wrong & clear).sum(), (wrong & ~clear).sum()))
    assert left_out <= LEFT_OUT_CAP[precision]
    assert not np.any(wrong & clear)


def test_refill_placement_and_split(g2048):
    for precision in ("f32", "bf16"):
        net = device_net("small", precision)
        ref = play(net, 2000, 2000, 0.25, 8, base=3)
        for waves in (1, 3):                                 # one wavefront plays all 2,000 games through its 32 slots
            assert_same(ref, play(net, 2000, 2000, 0.25, 8, base=3, max_waves=waves), "small %s, max_waves=%d" % (precision, waves))
    net = device_net("fixture", "bf16")
    ref = play(net, 2000, 2000, 0.0, 8, base=3)
    assert_same(ref, play(net, 2000, 2000, 0.0, 8, base=3, max_waves=3), "fixture, max_waves=3")
    net = device_net("fixture", "f32")
    whole = play(net, 2000, 2000, 0.25, 9, base=1 << 33)
    assert_same(whole, play(net, 2000, 2000, 0.25, 9, base=1 << 33), "two launches")
    lo = play(net, 1000, 2000, 0.25, 9, base=1 << 33)
    hi = play(net, 1000, 2000, 0.25, 9, base=(1 << 33) + 1000)
    for k in KEYS:
        assert torch.equal(torch.cat([lo[k], hi[k]]), whole[k]), "split at 1000: %s differs" % k


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_canaries_and_one_move(g2048, precision):
    from g2048 import _lib as L
    from g2048 import ops
    from g2048.vec import VecGame2048
    net = device_net("fixture", precision)
    epsilon = 0.25
    for n in (77, 300):
        for cap in (1, 50):
            extra = 37
            env = VecGame2048(n + extra, device=torch.device(DEV), seed=3)
            boards, scores = env.boards.clone(), env.scores.clone()
            outs = {"moves": torch.full((n + extra,), -7, dtype=torch.int32, device=DEV),
                    "valid": torch.full((n + extra,), -7, dtype=torch.int32, device=DEV),
                    "invalid": torch.full((n + extra,), -7, dtype=torch.int32, device=DEV),
                    "ms": torch.full((n + extra, 8), -7, dtype=torch.int32, device=DEV),
                    "reward": torch.full((n + extra,), -7.0, dtype=torch.float64, device=DEV),
                    "alive": torch.full((n + extra,), 7, dtype=torch.uint8, device=DEV),
                    "actions": torch.full((n + extra, cap), 7, dtype=torch.uint8, device=DEV)}
            ws = torch.empty(L.lib().g2048_play_qnet_workspace(n), dtype=torch.uint8, device=DEV)
            opts = L.POLICY_BF16 if precision == "bf16" else L.POLICY_F32
            L.call(torch.device(DEV), L.lib().g2048_play_qnet_games, boards.data_ptr(), scores.data_ptr(), net.packed.data_ptr(),
                   net.dim_ff, net.n_layers, outs["moves"].data_ptr(), outs["valid"].data_ptr(), outs["invalid"].data_ptr(),
                   outs["ms"].data_ptr(), outs["reward"].data_ptr(), outs["alive"].data_ptr(), outs["actions"].data_ptr(), cap, epsilon, 3,
                   0, n, opts, 0, ws.data_ptr(), ws.numel(), L.stream_ptr(torch.device(DEV)))
            torch.cuda.synchronize()
            assert torch.equal(boards[n:], env.boards[n:]) and torch.equal(scores[n:], env.scores[n:])
            for k, v in outs.items():
                assert bool((v[n:] == (7 if k in ("alive", "actions") else -7)).all()), "%s written past n = %d" % (k, n)
            ref = play(net, n, cap, epsilon, 3)
            assert torch.equal(outs["moves"][:n], ref["moves"]) and torch.equal(outs["actions"][:n], ref["actions"])
            assert torch.equal(boards[:n], ref["boards"]) and torch.equal(outs["reward"][:n], ref["reward_sum"])
            assert torch.equal(outs["ms"][:n], ref["milestone_move"]) and torch.equal(outs["alive"][:n], ref["alive"])
            assert torch.equal(outs["valid"][:n], ref["valid_moves"]) and torch.equal(outs["invalid"][:n], ref["invalid_moves"])
            if cap == 1:
                assert bool((outs["moves"][:n] == 1).all()) and bool((outs["alive"][:n] == 1).all())
    with pytest.raises(ValueError, match="blob of"):
        env = VecGame2048(4, device=torch.device(DEV), seed=3)
        ops.play_qnet_games(env.boards, env.scores, net.packed[:-16].contiguous(), net.dim_ff, net.n_layers, precision)


def test_evaluate_qnet_histories_drivers_and_refresh(g2048):
    import copy
    from g2048 import DeviceQNetwork
    net = DeviceQNetwork(copy.deepcopy(hash_model("fixture")).float().to(DEV), precision="f32")
    kw = dict(num_games=300, max_moves=2000, epsilon=0.25, seed=17, game_id_base=40)
    res = g2048.evaluate_qnet(net, histories="best5", **kw)
    ref = g2048.evaluate_qnet(net, fused=False, **kw)
    for k in ("scores", "highest_tiles", "moves", "valid_moves", "invalid_moves", "milestones", "milestones_by_game", "best_games",
              "best_score", "best_game_idx", "unfinished", "total_moves", "total_expansions", "episode_rewards", "parameters"):
        assert res[k] == ref[k], k
    assert set(res) - {"games"} == set(ref)
    assert np.array_equal(res["final_boards"], ref["final_boards"]) and np.array_equal(res["best_board"], ref["best_board"])
    assert res["parameters"] == {"epsilon": 0.25, "precision": "f32", "max_moves": 2000, "num_games": 300, "seed": 17}
    assert sorted(res["games"]) == sorted(res["best_games"])
    for i, game in res["games"].items():
        assert np.array_equal(game["board_history"][-1], res["final_boards"][i])
        assert game["scores_history"][-1] == res["scores"][i] and len(game["moveset"]) == res["moves"][i]
    print(res["summary"])
    with pytest.raises(ValueError, match="lives on"):
        g2048.evaluate_qnet(net, 4, device="cuda:%d" % (torch.cuda.device_count() + 1))
    with torch.no_grad():
        net.model.fc.weight.mul_(-1.0)
    assert g2048.evaluate_qnet(net, **kw)["moves"] == res["moves"]               # the packed weights are what plays
    net.refresh()
    assert g2048.evaluate_qnet(net, **kw)["moves"] != res["moves"]
