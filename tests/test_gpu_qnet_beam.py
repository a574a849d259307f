"""The hybrid agent's beam search on the MI355X: g2048_qnet_beam_actions and g2048_qnet_beam_expand against what the reference's
own DQNAgent.beam_search recorded (tests/golden/qnet_beam.npz), DeviceQNetwork.act_beam at search_depth 1 against the plain
restatement (tests/qnet_beam_ref.py) on the device's own Q-values, the epsilon coin against g2048_qnet_select_actions, and
g2048_play_qnet_beam_games against the unfused loop (every output, bit for bit) and, move by move, against the restatement.
The game tests play and compare through tests/play_harness.py, as the other three game kernels' tests do; the Q-network
builder is tests/test_gpu_qnet_play.py's (the fixture's network, the small one, and dim_ff 96 with 3 layers). Everything is exact: the decision is integer and f64 arithmetic in a fixed order,
and the forward's accuracy is pinned elsewhere (tests/test_gpu_qnet.py)."""
from functools import partial

import numpy as np
import pytest
import torch

import play_harness as H
import qnet_beam_ref as R
import qnet_weights as qw
from conftest import load_golden
from play_harness import DEV, g2048  # noqa: F401
from test_gpu_qnet_play import device_net
from test_policy_host import random_boards

pytestmark = pytest.mark.gpu

REFERENCE = (15, 30, 64)            # DQNAgent's beam_width, search_depth, beam_search_threshold
EARLY = (4, 2, 8)                   # a narrow beam that plans from the first 8 on: other arguments, many planned moves


@pytest.fixture(scope="module")
def golden():
    return load_golden("qnet_beam.npz")


def canaried(n, shape=(), dtype=torch.uint8, pad=13):
    """(whole, view of the first n rows): the rows past n hold 9 and must still hold it afterwards."""
    whole = torch.full((n + pad,) + tuple(shape), 9, dtype=dtype, device=DEV)
    return whole, whole[:n]


def untouched(*wholes_n):
    return all(bool((w[n:] == 9).all()) for w, n in wholes_n)


def leaf_as_q(leaf):
    q = np.repeat(np.asarray(leaf, np.float32)[..., None], 4, axis=-1)
    q[..., 1:] -= np.float32(1.0)
    return np.ascontiguousarray(q)


def test_beam_actions_at_depth_30_equal_the_reference(g2048, golden):
    from g2048 import ops
    net = device_net("fixture", "f32")
    boards, planned, action = golden["d30_board"], golden["d30_planned"], golden["d30_action"]
    threshold = int(golden["threshold"])
    b = torch.from_numpy(boards).to(DEV)
    greedy, q = [x.clone() for x in net.act(b)]
    greedy = greedy.cpu().numpy()
    total = len(boards)
    for n in (1, 31, 33, 129, total):
        for wi, w in enumerate(golden["d30_widths"]):
            (wa, a), (wp, p), (we, e) = canaried(n), canaried(n), canaried(n)
            ops.qnet_beam_actions(q[:n], b[:n], None, int(w), 30, threshold, 0.99, actions=a, planned=p, explored=e)
            torch.cuda.synchronize()
            assert untouched((wa, n), (wp, n), (we, n)), "rows past n were written (n %d)" % n
            got, pl = a.cpu().numpy(), planned[:n] == 1
            assert np.array_equal(p.cpu().numpy(), planned[:n]) and not e.cpu().numpy().any()
            assert np.array_equal(got[pl], action[wi, :n][pl]), "width %d, n %d: planned actions differ from the reference" % (w, n)
            assert np.array_equal(got[~pl], greedy[:n][~pl]), "width %d, n %d: an un-planned board is not the exploit action" % (w, n)
    # search_depth 2 is search_depth 30; succ_q is not read there; the threshold moves the planned set
    a30, _, _ = ops.qnet_beam_actions(q, b, None, 15, 30, threshold)
    a2, _, _ = ops.qnet_beam_actions(q, b, torch.full((total, 32, 4), float("nan"), device=DEV), 15, 2, threshold)
    assert torch.equal(a30, a2)
    _, p8, _ = ops.qnet_beam_actions(q, b, None, 15, 30, 8)
    assert np.array_equal(p8.cpu().numpy(), np.array([R.planned(x, 8) for x in boards], np.uint8)) and int(p8.sum()) > int(planned.sum())
    a_net, q_net = net.act_beam(b)                          # the same through DeviceQNetwork.act_beam at the reference's settings
    assert torch.equal(a_net, a30) and torch.equal(q_net, q)


def test_depth_1_decision_and_expansion_equal_the_reference(g2048, golden):
    from g2048 import ops
    net = device_net("fixture", "f32")
    boards, gamma, seed = golden["d1_board"], float(golden["gamma"]), int(golden["seed"])
    n = len(boards)
    b = torch.from_numpy(boards).to(DEV)
    q = net(b).clone()
    zeros = torch.zeros(n, dtype=torch.uint8, device=DEV)
    for s in range(2):
        step = int(golden["d1_steps"][s])
        (ws, succ), (wc, count) = canaried(n, (32, 16)), canaried(n, (4,))
        ops.qnet_beam_expand(b, seed, step, 0, succ=succ, count=count)
        torch.cuda.synchronize()
        assert untouched((ws, n), (wc, n))
        assert np.array_equal(succ.cpu().numpy(), golden["d1_succ"][s]) and np.array_equal(count.cpu().numpy(), golden["d1_count"][s])
        sim, _, _, sim_count = ops.simulate_move_sampled(b, zeros, seed, step, 0)             # action 0: the very same successors
        assert torch.equal(succ[:, :8], sim) and torch.equal(count[:, 0], sim_count)
        succ_q = torch.from_numpy(leaf_as_q(golden["d1_leaf"][s])).to(DEV)
        for wi, w in enumerate(golden["d1_widths"]):
            a, p, e = ops.qnet_beam_actions(q, b, succ_q, int(w), 1, int(golden["threshold"]), gamma)
            assert np.array_equal(a.cpu().numpy(), golden["d1_action"][s, wi]), "draw set %d width %d" % (s, w)
            assert bool(p.all()) and not bool(e.any())
    # ids: board i under id_base k is board i + k under id_base 0
    s1, c1 = ops.qnet_beam_expand(b[5:], seed, 5, 5)
    s0, c0 = ops.qnet_beam_expand(b, seed, 5, 0)
    assert torch.equal(s1, s0[5:]) and torch.equal(c1, c0[5:])
    big, _ = ops.qnet_beam_expand(b[:33], seed, 5, (1 << 40) + 3)
    assert not torch.equal(big, s0[:33])


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_act_beam_at_depth_1_equals_the_restatement_on_the_device_q(g2048, golden, precision):
    from g2048 import ops
    net = device_net("fixture", precision)
    boards = np.concatenate([golden["d1_board"][:150], np.minimum(random_boards(120, 3), 5), golden["d30_board"][-40:]])
    n, seed, step, base, width = len(boards), 77, 9, (1 << 33) + 11, 15
    b = torch.from_numpy(boards).to(DEV)
    actions, q = [x.clone() for x in net.act_beam(b, 0.0, seed, step, base, beam_width=width, search_depth=1)]
    succ, count = ops.qnet_beam_expand(b, seed, step, base)
    leaf = net(succ.view(n * 32, 16)).clone().view(n, 32, 4).max(dim=2).values.cpu().numpy()
    assert torch.equal(q, net(b))
    q, got = q.cpu().numpy(), actions.cpu().numpy()
    planned = np.array([R.planned(x) for x in boards])
    assert 100 <= planned.sum() <= n - 50
    want = np.array([R.action(x, width, 1, 0.99, leaf[i]) if planned[i] else R.exploit(q[i], x) for i, x in enumerate(boards)], np.uint8)
    assert np.array_equal(got, want)
    d30 = net.act_beam(b, beam_width=width)[0].cpu().numpy()
    assert (d30 != got)[planned].mean() >= 0.1            # depth 1 is another decision (the fixture: 60 %), not the same one relabelled
    # the expansion the decision saw is the one with these keys: another step index moves some decisions
    other = net.act_beam(b, 0.0, seed, step + 1, base, beam_width=width, search_depth=1)[0].cpu().numpy()
    assert np.array_equal(other[~planned], got[~planned])


def test_epsilon_is_select_actions_own(g2048, golden):
    from g2048 import ops
    net = device_net("fixture", "f32")
    boards = np.concatenate([golden["d30_board"][:1500], golden["d30_board"][-700:]])
    b = torch.from_numpy(boards).to(DEV)
    q = net(b).clone()
    seed, t, base = 0x5EED, 1234, (1 << 33) + 5
    exploit, planned, none = [x.clone() for x in ops.qnet_beam_actions(q, b, None, *REFERENCE, 0.99, 0.0, seed, t, base)]
    assert not bool(none.any()) and 0 < int(planned.sum()) < len(boards)
    for epsilon in (0.25, 1.0):
        a, p, e = ops.qnet_beam_actions(q, b, None, *REFERENCE, 0.99, epsilon, seed, t, base)
        sa, se = ops.qnet_select_actions(q, b, epsilon, seed, t, base)
        assert torch.equal(e, se) and torch.equal(p, planned)
        ex = e.bool()
        assert torch.equal(a[ex], sa[ex]) and torch.equal(a[~ex], exploit[~ex])
        assert int(ex.sum()) == len(boards) if epsilon == 1.0 else 0.15 * len(boards) < int(ex.sum()) < 0.35 * len(boards)
    assert bool((exploit != ops.qnet_select_actions(q, b, 0.0, seed, t, base)[0]).any())


play, play_beam = partial(H.play, H.QNET), partial(H.play, H.QNET_BEAM)


FUSED_CASES = ([(e, p, w) for w in ("fixture", "small") for p in ("f32", "bf16") for e in (0.0, 0.05)]
               + [(0.05, p, "odd") for p in ("f32", "bf16")])


@pytest.mark.parametrize("epsilon,precision,network", FUSED_CASES, ids=["%s-%s-%s" % c for c in FUSED_CASES])
def test_fused_beam_games_equal_the_unfused_loop(g2048, epsilon, precision, network):
    net = device_net(network, precision)
    for n, cap, beam in ((300, 160, REFERENCE), (33, 400, REFERENCE), (77, 60, EARLY)):
        seed = 2000 + n + cap
        a = play_beam(net, n, cap, (epsilon,) + beam, seed, fused=False)
        b = play_beam(net, n, cap, (epsilon,) + beam, seed, fused=True)
        H.assert_same(a, b, "epsilon %g %s %s n=%d cap=%d beam %s" % (epsilon, precision, network, n, cap, beam))
        H.check_game_invariants(b, cap)
        assert int((b["milestone_move"][:, 0] >= 0).sum()) > 0 or beam is EARLY, "no game reached 64: the search never planned"


@pytest.mark.parametrize("precision,beam", [("f32", REFERENCE), ("bf16", REFERENCE), ("f32", EARLY)])
def test_recorded_beam_games_carry_the_restatements_actions(g2048, oracle, precision, beam):
    """Every pre-move board of 64 games at epsilon 0: a planned board carries the restatement's action, every other board the
    exploit action of a fresh forward on it."""
    net = device_net("fixture", precision)
    n, seed, cap = 64, 777, 250
    r = play_beam(net, n, cap, (0.0,) + beam, seed)
    bh, _, q, longest = H.replay(H.QNET_BEAM, net, r, seed, True)
    moves, acts = r["moves"].cpu().numpy(), r["actions"].cpu().numpy()
    live = np.arange(longest)[None, :] < moves[:, None]
    pos = bh[:, :longest][live]
    got = acts[:, :longest][live]
    greedy = qw.masked_argmax(q[live], qw.mask_bits(oracle.valid_moves_batch(pos)))
    planned = np.array([R.planned(x, beam[2]) for x in pos])
    want = greedy.copy()
    want[planned] = [R.action(x, beam[0]) for x in pos[planned]]
    assert np.array_equal(got, want)
    games_planned = sum(bool(np.any([R.planned(x, beam[2]) for x in bh[g, :moves[g]]])) for g in range(0, n, 8))
    print("%s beam %s: %d positions, %d planned, %d of them not the exploit action" % (
        precision, beam, len(pos), planned.sum(), (want != greedy)[planned].sum()))
    assert planned.sum() > 0 and games_planned > 0, "no game reached a planned position"
    assert (want != greedy)[planned].any(), "every planned action is the exploit action: the test proves nothing"
    assert (~planned).sum() > 0


def test_games_without_the_search_are_what_they_were(g2048):
    """g2048_play_qnet_games after its kernel gained the template parameter: still its own unfused loop, bit for bit, and not
    the games of the search."""
    for precision in ("f32", "bf16"):
        net = device_net("fixture", precision)
        a = play(net, 300, 160, 0.05, 4321, fused=False)
        b = play(net, 300, 160, 0.05, 4321, fused=True)
        H.assert_same(a, b, "no search, %s" % precision)
        c = play_beam(net, 300, 160, (0.05,) + REFERENCE, 4321)
        assert not torch.equal(b["actions"], c["actions"])


def test_evaluate_qnet_with_the_search(g2048):
    net = device_net("small", "f32")
    kw = dict(num_games=96, max_moves=200, epsilon=0.01, seed=99, use_beam_search=True)
    fused = g2048.evaluate_qnet(net, **kw)
    loop = g2048.evaluate_qnet(net, fused=False, **kw)
    for k in ("scores", "moves", "highest_tiles", "episode_rewards", "final_boards"):
        assert np.array_equal(np.asarray(fused[k]), np.asarray(loop[k])), k
    p = fused["parameters"]
    assert (p["use_beam_search"], p["beam_width"], p["search_depth"], p["beam_search_threshold"], p["gamma"]) == (True, 15, 30, 64, 0.99)
    plain = g2048.evaluate_qnet(net, num_games=96, max_moves=200, epsilon=0.01, seed=99)
    assert sorted(plain["parameters"]) == ["epsilon", "max_moves", "num_games", "precision", "seed"]      # without the search: as before
    assert list(plain["moves"]) != list(fused["moves"])
    one = g2048.evaluate_qnet(net, num_games=40, max_moves=60, seed=99, use_beam_search=True, search_depth=1, beam_search_threshold=8,
                              fused=False)
    two = g2048.evaluate_qnet(net, num_games=40, max_moves=60, seed=99, use_beam_search=True, search_depth=2, beam_search_threshold=8,
                              fused=False)
    assert one["parameters"]["search_depth"] == 1 and list(one["scores"]) != list(two["scores"])
    with pytest.raises(ValueError, match="fused=False"):
        g2048.evaluate_qnet(net, num_games=4, use_beam_search=True, search_depth=1)
