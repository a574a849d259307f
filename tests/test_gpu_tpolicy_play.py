"""g2048_play_tpolicy_games on the MI355X: the fused kernel against the unfused loop of existing launches (every output, bit
for bit), the recorded decisions against the CPU oracle and against tpolicy.forward_reference in float64, independence of the
block count and of the id split, canaries past n, and evaluate_policy with a DeviceTransformerPolicy. The checks themselves are
tests/play_harness.py's, shared with the other three game kernels; this file holds the networks, the shapes, the seeds and the
bounds.

The networks carry the hash-derived weights of tests/tpolicy_weights.py: the fixture's (dim_ff 2048, 2 layers), a small one
(dim_ff 32, 1 layer), the bench shape (dim_ff 128, 2 layers) and one that is no power of two (dim_ff 96, 3 layers: an odd number
of 32-feature slices and a third layer's offsets in the packed blob)."""
from functools import partial

import pytest
import torch

import play_harness as H
import tpolicy_weights as tw
from play_harness import DEV, g2048  # noqa: F401
from test_tpolicy_host import RefSpelling

pytestmark = pytest.mark.gpu

SHAPES = {"fixture": (2048, 2), "small": (32, 1), "bench": (128, 2), "odd": (96, 3)}
FUSED_CASES = ([(m, p, w) for w in ("fixture", "small") for p in ("f32", "bf16") for m in ("masked", "unmasked", "greedy")]
               + [("masked", p, "odd") for p in ("f32", "bf16")])
_MODELS, _POLICIES = {}, {}


def hash_model(network):
    """RefSpelling of the network's shape in float64 eval mode, on the CPU, carrying the hash-derived weights."""
    if network not in _MODELS:
        dim_ff, n_layers = SHAPES[network]
        model = RefSpelling(dim_ff, n_layers).double()
        shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        assert shapes == tw.reference_shapes(dim_ff, n_layers)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in tw.state_dict(shapes).items()})
        _MODELS[network] = model.eval()
    return _MODELS[network]


def policy(network, precision):
    key = (network, precision)
    if key not in _POLICIES:
        import copy
        from g2048 import DeviceTransformerPolicy
        _POLICIES[key] = DeviceTransformerPolicy(copy.deepcopy(hash_model(network)).float().to(DEV), precision=precision)
    return _POLICIES[key]


play = partial(H.play, H.TPOLICY)


@pytest.mark.parametrize("mode,precision,network", FUSED_CASES, ids=["%s-%s-%s" % c for c in FUSED_CASES])
def test_fused_equals_unfused(g2048, mode, precision, network):
    pol = policy(network, precision)
    for n, cap in ((1, 2000), (15, 2000), (17, 2000), (4097, 2000), (4097, 37)):
        seed = 1000 + n + cap
        a = play(pol, n, cap, mode, seed, fused=False)
        b = play(pol, n, cap, mode, seed, fused=True)
        H.assert_same(a, b, "%s %s %s n=%d cap=%d" % (mode, precision, network, n, cap))
        H.check_game_invariants(b, cap)


def test_fused_equals_unfused_65536(g2048):
    pol = policy("bench", "f32")
    a = play(pol, 65536, 2000, "masked", 77, base=12345, fused=False)
    b = play(pol, 65536, 2000, "masked", 77, base=12345, fused=True)
    H.assert_same(a, b, "65536 games")
    m = b["moves"].double()
    print("hash weights dim_ff 128, masked, f32: mean game %.1f moves, longest %d" % (m.mean().item(), int(m.max().item())))


@pytest.mark.parametrize("mode", ["masked", "unmasked"])
def test_decisions_and_moves_against_the_oracle(g2048, oracle, mode):
    """256 complete games: replaying the recorded actions with the oracle's env step gives g2048_replay_games' histories and
    the kernel's final state, counters, milestones and f64 reward sums; the oracle's sampler on the device forward's
    probabilities of every pre-move board gives the recorded action of every move."""
    pol = policy("fixture", "f32")
    n, seed = 256, 4242
    r = play(pol, n, 2000, mode, seed)
    bh, sh, probs, _ = H.replay(H.TPOLICY, pol, r, seed, True)
    H.check_games_against_oracle(oracle, r, (bh, sh), seed, lambda t, boards, mask, live: oracle.sample_batch(
        probs[:, t], mask if mode == "masked" else None, seed, t, 0))


GAP_BOUND = 6e-5          # 3 x the 2e-5 per-probability bound tests/test_gpu_tpolicy.py holds the f32 forward to
RATE_BOUND = 1e-3         # a draw falls within 6e-5 of one of at most three boundaries with probability <= 3.6e-4


@pytest.mark.parametrize("mode", ["masked", "unmasked"])
def test_fixture_network_in_f64(g2048, oracle, mode):
    """The fixture network in f32 against tpolicy.forward_reference in float64 plus the oracle's sampling: a different decision
    is allowed only where the draw lies within 6e-5 (relative to the CDF total) of a CDF boundary, and at most 1e-3 of all
    decisions may differ."""
    from g2048 import tpolicy
    parsed = tpolicy.parse(hash_model("fixture"))
    pol = policy("fixture", "f32")
    n, seed = 256, 99
    r = play(pol, n, 2000, mode, seed)
    bh = H.replay(H.TPOLICY, pol, r, seed, False)[0]

    def probs_f64(boards):
        tb = torch.from_numpy(boards)
        return torch.cat([tpolicy.forward_reference(parsed, tb[i:i + 4096])[0] for i in range(0, len(tb), 4096)]).numpy()
    H.check_decisions_against_f64(oracle, r, bh, seed, mode == "masked", probs_f64, GAP_BOUND, RATE_BOUND, what=mode)


def test_refill_and_placement_independence(g2048):
    H.check_independence(H.TPOLICY, policy("small", "bf16"), 2000, 2000, "masked", 8, 3, units=(1, 3))
    pol = policy("fixture", "f32")
    H.check_independence(H.TPOLICY, pol, 2000, 2000, "masked", 8, 3, units=(3,), what="fixture,")
    H.check_independence(H.TPOLICY, pol, 2000, 2000, "unmasked", 9, 1 << 33, split=1000)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_canaries_and_one_move(g2048, precision):
    from g2048 import ops
    from g2048.vec import VecGame2048
    pol = policy("fixture", precision)
    H.check_canaries(H.TPOLICY, pol, "masked", [(n, cap) for n in (77, 300) for cap in (1, 50)])
    with pytest.raises(ValueError, match="blob of"):
        env = VecGame2048(4, device=torch.device(DEV), seed=3)
        ops.play_tpolicy_games(env.boards, env.scores, pol.packed[:-16].contiguous(), pol.dim_ff, pol.n_layers, precision)


def test_evaluate_policy_histories_drivers_and_refresh(g2048):
    import copy
    from g2048 import DeviceTransformerPolicy
    pol = DeviceTransformerPolicy(copy.deepcopy(hash_model("fixture")).float().to(DEV), precision="f32")
    kw = dict(num_games=300, max_moves=2000, mode="masked", seed=17, game_id_base=40)
    res = H.check_evaluate_drivers(g2048.evaluate_policy, pol, kw,
                                   {"mode": "masked", "precision": "f32", "max_moves": 2000, "num_games": 300, "seed": 17})
    with torch.no_grad():
        pol.model.actor.weight.mul_(-1.0)
    assert g2048.evaluate_policy(pol, **kw)["moves"] == res["moves"]             # the packed weights are what plays
    pol.refresh()
    assert g2048.evaluate_policy(pol, **kw)["moves"] != res["moves"]
