"""g2048_qnet_select_actions and g2048_play_qnet_games on the MI355X: the select launch against a NumPy restatement of
DQNAgent.select_action, the fused kernel against the unfused loop of the launches that exist apart from it (every output, bit
for bit), the recorded games against the CPU oracle and the recorded decisions against the NumPy select_action on the device
forward's own Q, the greedy decisions against qnet.forward_reference in float64, independence of the wavefront count and of
the id split, canaries past n, and evaluate_qnet. The checks the game kernels have in common are tests/play_harness.py's; this
file holds the networks, the shapes, the seeds, the bounds, select_action in NumPy and the tests that have no sibling.

The networks carry the hash-derived weights of tests/qnet_weights.py: the fixture's (dim_ff 2048, 2 layers), a small one
(dim_ff 32, 1 layer) and one that is no power of two (dim_ff 96, 3 layers: an odd number of 32-feature slices and a third layer's
offsets in the packed blob)."""
from functools import partial

import numpy as np
import pytest
import torch

import play_harness as H
import qnet_weights as qw
from play_harness import DEV, g2048  # noqa: F401
from test_gpu_qnet import LEFT_OUT_CAP, module_rows_f32, q_bound
from test_policy_host import random_boards
from test_qnet_host import RefSpelling, bf16_round, golden_model

pytestmark = pytest.mark.gpu

_MODELS, _NETS = {}, {}
SHAPES = {"small": (32, 1), "odd": (96, 3)}
FUSED_CASES = ([(e, p, w) for w in ("fixture", "small") for p in ("f32", "bf16") for e in (0.0, 0.25, 1.0)]
               + [(0.25, p, "odd") for p in ("f32", "bf16")])

DEAD = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1]                 # full, no merge: no valid move
ONLY_RIGHT = [1, 2, 1, 0, 2, 1, 2, 0, 1, 2, 1, 0, 2, 1, 2, 0]
ONLY_DOWN = [3, 4, 3, 4, 4, 3, 4, 3, 3, 4, 3, 4, 0, 0, 0, 0]
BIASED_LEFT_UP = [0, 0, 0, 0, 0, 0, 1, 2, 0, 1, 2, 3, 0, 2, 3, 7]       # 128 in the corner; neither RIGHT nor DOWN moves anything
BIASED_LEFT_RIGHT = [1, 1, 2, 3, 2, 3, 1, 2, 1, 2, 3, 1, 2, 1, 2, 8]    # 256 in the corner; full, one horizontal pair


def hash_model(network):
    """RefSpelling in float64 eval mode, on the CPU, carrying the hash-derived weights: the fixture's network or one of SHAPES."""
    if network not in _MODELS:
        if network == "fixture":
            model = golden_model()[2]
        else:
            model = RefSpelling(*SHAPES[network]).double()
            shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
            assert shapes == qw.reference_shapes(*SHAPES[network])
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


play = partial(H.play, H.QNET)


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


@pytest.mark.parametrize("epsilon,precision,network", FUSED_CASES, ids=["%s-%s-%s" % c for c in FUSED_CASES])
def test_fused_equals_unfused(g2048, epsilon, precision, network):
    net = device_net(network, precision)
    for n, cap in ((1, 2000), (31, 2000), (33, 2000), (129, 2000), (4097, 2000), (4097, 37)):
        seed = 1000 + n + cap
        a = play(net, n, cap, epsilon, seed, fused=False)
        b = play(net, n, cap, epsilon, seed, fused=True)
        H.assert_same(a, b, "epsilon %g %s %s n=%d cap=%d" % (epsilon, precision, network, n, cap))
        H.check_game_invariants(b, cap)
        if n == 4097 and cap == 2000:
            m = b["moves"].double()
            print("%s %s epsilon %g: mean game %.1f moves, longest %d" % (network, precision, epsilon, m.mean().item(), int(m.max().item())))


def test_recorded_games_against_the_oracle(g2048, oracle):
    """256 complete games at epsilon 0.25: replaying the recorded actions with the oracle's env step gives g2048_replay_games'
    histories and the kernel's final state, counters, milestones and f64 reward sums; the NumPy select_action on the device
    forward's Q of every pre-move board gives the recorded action of every move."""
    net = device_net("fixture", "f32")
    n, seed, epsilon = 256, 4242, 0.25
    r = play(net, n, 2000, epsilon, seed)
    bh, sh, q, _ = H.replay(H.QNET, net, r, seed, True)
    notes = H.check_games_against_oracle(oracle, r, (bh, sh), seed, lambda t, boards, mask, live: select_action_np(
        oracle, q[:, t], boards, mask, epsilon, seed, t, 0))
    decisions = int(r["moves"].sum())
    explored_all = sum(int((live & explored).sum()) for live, (explored, biased) in notes)
    explored_biased = sum(int((live & explored & biased).sum()) for live, (explored, biased) in notes)
    print("%d decisions, %d explored, %d of them with the biased preferences" % (decisions, explored_all, explored_biased))
    assert explored_biased > 0 and 0.2 * decisions < explored_all < 0.3 * decisions


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
    bh, _, _, longest = H.replay(H.QNET, net, r, seed, False)
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
    for precision in ("f32", "bf16"):                        # one wavefront plays all 2,000 games through its 32 slots
        H.check_independence(H.QNET, device_net("small", precision), 2000, 2000, 0.25, 8, 3, units=(1, 3), what="small %s," % precision)
    H.check_independence(H.QNET, device_net("fixture", "bf16"), 2000, 2000, 0.0, 8, 3, units=(3,), what="fixture,")
    H.check_independence(H.QNET, device_net("fixture", "f32"), 2000, 2000, 0.25, 9, 1 << 33, split=1000)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_canaries_and_one_move(g2048, precision):
    from g2048 import ops
    from g2048.vec import VecGame2048
    net = device_net("fixture", precision)
    H.check_canaries(H.QNET, net, 0.25, [(n, cap) for n in (77, 300) for cap in (1, 50)])
    with pytest.raises(ValueError, match="blob of"):
        env = VecGame2048(4, device=torch.device(DEV), seed=3)
        ops.play_qnet_games(env.boards, env.scores, net.packed[:-16].contiguous(), net.dim_ff, net.n_layers, precision)


def test_evaluate_qnet_histories_drivers_and_refresh(g2048):
    import copy
    from g2048 import DeviceQNetwork
    net = DeviceQNetwork(copy.deepcopy(hash_model("fixture")).float().to(DEV), precision="f32")
    kw = dict(num_games=300, max_moves=2000, epsilon=0.25, seed=17, game_id_base=40)
    res = H.check_evaluate_drivers(g2048.evaluate_qnet, net, kw,
                                   {"epsilon": 0.25, "precision": "f32", "max_moves": 2000, "num_games": 300, "seed": 17})
    with pytest.raises(ValueError, match="lives on"):
        g2048.evaluate_qnet(net, 4, device="cuda:%d" % (torch.cuda.device_count() + 1))
    with torch.no_grad():
        net.model.fc.weight.mul_(-1.0)
    assert g2048.evaluate_qnet(net, **kw)["moves"] == res["moves"]               # the packed weights are what plays
    net.refresh()
    assert g2048.evaluate_qnet(net, **kw)["moves"] != res["moves"]
