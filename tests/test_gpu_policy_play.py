"""g2048_play_policy_games on the MI355X: the fused kernel against the unfused loop of existing launches (every output, bit for
bit), the recorded decisions against the CPU oracle and against a NumPy f64 forward of the reference checkpoint, the
reference's batch-of-one rule, independence of the wavefront count and of the id split, canaries past n, and histories.
The checks themselves are tests/play_harness.py's, shared with the other three game kernels; this file holds the networks, the
shapes, the seeds and the bounds."""
from functools import partial

import numpy as np
import pytest
import torch

import play_harness as H
from play_harness import g2048  # noqa: F401
from test_policy_host import RefLayout, golden_modules, numpy_forward, perturb_bn, state_dict_np

pytestmark = pytest.mark.gpu

_POLICIES = {}


def random_actor():
    gen = torch.Generator().manual_seed(21)
    torch.manual_seed(21)
    return perturb_bn(RefLayout(4), gen)


def policy(weights, precision, batchnorm="auto"):
    key = (weights, precision, batchnorm)
    if key not in _POLICIES:
        from g2048 import DevicePolicy
        actor = golden_modules()[1] if weights == "reference" else random_actor()
        _POLICIES[key] = DevicePolicy(actor.to(H.DEV), precision=precision, batchnorm=batchnorm)
    return _POLICIES[key]


play = partial(H.play, H.POLICY)


@pytest.mark.parametrize("weights", ["reference", "random"])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ["masked", "unmasked", "greedy"])
def test_fused_equals_unfused(g2048, mode, precision, weights):
    pol = policy(weights, precision)
    for n, cap in ((1, 2000), (63, 2000), (65, 2000), (4097, 2000), (4097, 37)):
        seed = 1000 + n + cap
        a = play(pol, n, cap, mode, seed, fused=False)
        b = play(pol, n, cap, mode, seed, fused=True)
        H.assert_same(a, b, "%s %s %s n=%d cap=%d" % (mode, precision, weights, n, cap))
        H.check_game_invariants(b, cap)


def test_fused_equals_unfused_65536(g2048):
    pol = policy("reference", "f32")
    a = play(pol, 65536, 2000, "masked", 77, base=12345, fused=False)
    b = play(pol, 65536, 2000, "masked", 77, base=12345, fused=True)
    H.assert_same(a, b, "65536 games")
    m = b["moves"].double()
    print("reference checkpoint, masked, f32: mean game %.1f moves, longest %d" % (m.mean().item(), int(m.max().item())))


@pytest.mark.parametrize("mode", ["masked", "unmasked"])
def test_decisions_and_moves_against_the_oracle(g2048, oracle, mode):
    """256 complete games: replaying the recorded actions with the oracle's env step gives g2048_replay_games' histories and
    the kernel's final state, counters, milestones and f64 reward sums; the oracle's sampler on the device forward's
    probabilities of every pre-move board gives the recorded action of every move."""
    pol = policy("reference", "f32")
    n, seed = 256, 4242
    r = play(pol, n, 2000, mode, seed)
    bh, sh, probs, _ = H.replay(H.POLICY, pol, r, seed, True)
    H.check_games_against_oracle(oracle, r, (bh, sh), seed, lambda t, boards, mask, live: oracle.sample_batch(
        probs[:, t], mask if mode == "masked" else None, seed, t, 0))


@pytest.mark.parametrize("mode", ["masked", "unmasked"])
def test_reference_network_in_f64(g2048, oracle, mode):
    """The reference checkpoint in f32 against a NumPy f64 forward of its batch-of-one weights plus the oracle's sampling:
    a different decision is allowed only where the draw lies within 1e-5 (relative) of a CDF boundary."""
    sd = state_dict_np(golden_modules()[1])
    pol = policy("reference", "f32")
    n, seed = 256, 99
    r = play(pol, n, 2000, mode, seed)
    bh = H.replay(H.POLICY, pol, r, seed, False)[0]
    H.check_decisions_against_f64(oracle, r, bh, seed, mode == "masked",
                                  lambda boards: numpy_forward(sd, boards.astype(np.float32) / np.float32(15), False, True), 1e-5,
                                  what=mode)


def test_batch_of_one_rule(g2048):
    """With perturbed BatchNorm statistics the reference layout plays with its batch-of-one weights: the games of
    batchnorm="never", not those of "always"."""
    auto, never, always = (policy("random", "f32", bn) for bn in ("auto", "never", "always"))
    a, b, c = (play(p, 512, 400, "masked", 5) for p in (auto, never, always))
    H.assert_same(a, b, "auto vs never")
    assert not torch.equal(a["actions"], c["actions"])


def test_refill_and_placement_independence(g2048):
    H.check_independence(H.POLICY, policy("random", "bf16"), 2000, 2000, "masked", 8, 3, units=(1, 3))
    H.check_independence(H.POLICY, policy("reference", "f32"), 4097, 600, "unmasked", 9, 1 << 33, units=(1, 3), split=1000)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_canaries_and_one_move(g2048, precision):
    H.check_canaries(H.POLICY, policy("reference", precision), "masked", ((77, 1), (300, 50)))


def test_evaluate_policy_histories_and_drivers(g2048):
    kw = dict(num_games=300, max_moves=2000, mode="masked", seed=17, game_id_base=40)
    H.check_evaluate_drivers(g2048.evaluate_policy, policy("reference", "f32"), kw,
                             {"mode": "masked", "precision": "f32", "max_moves": 2000, "num_games": 300, "seed": 17})
