"""g2048_play_policy_games on the MI355X: the fused kernel against the unfused loop of existing launches (every output, bit for
bit), the recorded decisions against the CPU oracle and against a NumPy f64 forward of the reference checkpoint, the
reference's batch-of-one rule, independence of the wavefront count and of the id split, canaries past n, and histories."""
import numpy as np
import pytest
import torch

from test_policy_host import RefLayout, golden_modules, numpy_forward, perturb_bn, state_dict_np

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("boards", "scores", "moves", "valid_moves", "invalid_moves", "milestone_move", "alive", "reward_sum", "actions")
_POLICIES = {}


@pytest.fixture(scope="module")
def g2048():
    import __graft_entry__ as ge
    ge.ensure_built()
    return ge.import_package()


def random_actor():
    gen = torch.Generator().manual_seed(21)
    torch.manual_seed(21)
    return perturb_bn(RefLayout(4), gen)


def policy(weights, precision, batchnorm="auto"):
    key = (weights, precision, batchnorm)
    if key not in _POLICIES:
        from g2048 import DevicePolicy
        actor = golden_modules()[1] if weights == "reference" else random_actor()
        _POLICIES[key] = DevicePolicy(actor.to(DEV), precision=precision, batchnorm=batchnorm)
    return _POLICIES[key]


def play(pol, n, max_moves, mode, seed, base=0, fused=True, max_waves=0):
    from g2048 import ops
    from g2048.evaluate import _play_policy_stepwise
    from g2048.vec import VecGame2048
    env = VecGame2048(n, device=torch.device(DEV), seed=seed, id_base=base)
    start = env.boards.clone()
    if fused:
        r = ops.play_policy_games(env.boards, env.scores, pol.actor.blob(1), pol.precision, max_moves, mode, seed, base,
                                  want_rewards=True, want_actions=True, max_waves=max_waves)
    else:
        r = _play_policy_stepwise(env, pol.actor.blob(1), pol.precision, max_moves, mode, seed, base)
    torch.cuda.synchronize()
    r.update(boards=env.boards, scores=env.scores, start=start)
    return r


def assert_same(a, b, what):
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), "%s: %s differ" % (what, k)


@pytest.mark.parametrize("weights", ["reference", "random"])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ["masked", "unmasked", "greedy"])
def test_fused_equals_unfused(g2048, mode, precision, weights):
    pol = policy(weights, precision)
    for n, cap in ((1, 2000), (63, 2000), (65, 2000), (4097, 2000), (4097, 37)):
        seed = 1000 + n + cap
        a = play(pol, n, cap, mode, seed, fused=False)
        b = play(pol, n, cap, mode, seed, fused=True)
        assert_same(a, b, "%s %s %s n=%d cap=%d" % (mode, precision, weights, n, cap))
        if cap == 37:
            assert int(b["alive"].sum()) > 0 and int((b["moves"] == 37).sum()) >= int(b["alive"].sum())
        assert int(b["moves"].min()) >= 1 and bool((b["valid_moves"] + b["invalid_moves"] == b["moves"]).all())


def test_fused_equals_unfused_65536(g2048):
    pol = policy("reference", "f32")
    a = play(pol, 65536, 2000, "masked", 77, base=12345, fused=False)
    b = play(pol, 65536, 2000, "masked", 77, base=12345, fused=True)
    assert_same(a, b, "65536 games")
    m = b["moves"].double()
    print("reference checkpoint, masked, f32: mean game %.1f moves, longest %d" % (m.mean().item(), int(m.max().item())))


def replay_and_forward(g2048, pol, r, seed):
    """Every pre-move board of every game (g2048_replay_games) and the actor's probabilities for it (g2048_policy_forward)."""
    from g2048 import ops
    longest = int(r["moves"].max().item())
    bh, sh, fh = ops.replay_games(r["start"], r["actions"], r["moves"], seed, longest=longest)
    k = bh.shape[0]
    probs = ops.policy_forward(bh[:, :longest].reshape(k * longest, 16).contiguous(), pol.actor.blob(1), None, pol.precision)
    torch.cuda.synchronize()
    return bh.cpu().numpy(), sh.cpu().numpy(), probs.view(k, longest, 4).cpu().numpy(), longest


@pytest.mark.parametrize("mode", ["masked", "unmasked"])
def test_decisions_and_moves_against_the_oracle(g2048, oracle, mode):
    """256 complete games: replaying the recorded actions with the oracle's env step gives g2048_replay_games' histories and
    the kernel's final state, counters, milestones and f64 reward sums; the oracle's sampler on the device forward's
    probabilities of every pre-move board gives the recorded action of every move."""
    pol = policy("reference", "f32")
    n, seed = 256, 4242
    r = play(pol, n, 2000, mode, seed)
    bh, sh, probs, longest = replay_and_forward(g2048, pol, r, seed)
    moves = r["moves"].cpu().numpy()
    acts = r["actions"].cpu().numpy()
    b = r["start"].cpu().numpy()
    sc = np.zeros(n, np.uint32)
    rsum = np.zeros(n, np.float64)
    ms = np.full((n, 8), -1, np.int64)
    valid = np.zeros(n, np.int64)
    for t in range(longest):
        live = t < moves
        assert np.array_equal(b[live], bh[live, t]) and np.array_equal(sc[live], sh[live, t].astype(np.uint32))
        mask = oracle.valid_moves_batch(b) if mode == "masked" else None
        sampled, _ = oracle.sample_batch(probs[:, t], mask, seed, t, 0)
        assert np.array_equal(sampled[live], acts[live, t]), "move %d: the oracle samples different actions" % t
        a = np.where(live, acts[:, t], 0).astype(np.uint8)
        nb, nsc, rw, fl = oracle.step_batch(b, a, sc, seed, t, 0)
        b = np.where(live[:, None], nb, b)
        sc = np.where(live, nsc, sc)
        rsum = np.where(live, rsum + rw, rsum)
        valid += (live & ((fl & 2) != 0)).astype(np.int64)
        code = (fl >> 3).astype(np.int64)
        for k in range(8):
            ms[:, k] = np.where(live & (ms[:, k] < 0) & (code >= 6 + k), t, ms[:, k])
    assert np.array_equal(b, r["boards"].cpu().numpy()) and np.array_equal(sc, r["scores"].cpu().numpy().astype(np.uint32))
    assert np.array_equal(rsum, r["reward_sum"].cpu().numpy()), "f64 reward sums differ"
    assert np.array_equal(valid, r["valid_moves"].cpu().numpy()) and np.array_equal(ms, r["milestone_move"].cpu().numpy())
    assert np.array_equal(moves - valid, r["invalid_moves"].cpu().numpy())


@pytest.mark.parametrize("mode", ["masked", "unmasked"])
def test_reference_network_in_f64(g2048, oracle, mode):
    """The reference checkpoint in f32 against a NumPy f64 forward of its batch-of-one weights plus the oracle's sampling:
    a different decision is allowed only where the draw lies within 1e-5 (relative) of a CDF boundary."""
    g, actor, _ = golden_modules()
    sd = state_dict_np(actor)
    pol = policy("reference", "f32")
    n, seed = 256, 99
    r = play(pol, n, 2000, mode, seed)
    bh, _, _, longest = replay_and_forward(g2048, pol, r, seed)
    moves = r["moves"].cpu().numpy()
    acts = r["actions"].cpu().numpy()
    decisions = disagree = 0
    for t in range(longest):
        live = t < moves
        boards = bh[live, t]
        p64 = numpy_forward(sd, boards.astype(np.float32) / np.float32(15), False, True)
        mask = oracle.valid_moves_batch(boards) if mode == "masked" else np.full(len(boards), 15, np.uint8)
        ids = np.nonzero(live)[0]
        k0, k1 = oracle.rng_keys(seed, oracle.DOM_POLICY, t)
        u = np.array([(oracle.rng_draw(k0, k1, int(i), 0) >> 8) for i in ids], np.float64) * 2.0 ** -24
        m = np.where(mask == 0, 15, mask)
        w = np.where((m[:, None] >> np.arange(4)) & 1, p64 + 1e-10, 0.0)
        cdf = np.cumsum(w, axis=1)
        x = u * cdf[:, 3]
        want = (x[:, None] >= cdf[:, :3]).sum(axis=1)
        top = np.array([int(v).bit_length() - 1 for v in m])          # rounding past the last valid action (sample_action)
        want = np.where((m >> want) & 1, want, top)
        got = acts[live, t]
        bad = want != got
        if bad.any():
            gap = np.abs(cdf[bad, :3] - x[bad, None]).min(axis=1) / cdf[bad, 3]
            assert (gap <= 1e-5).all(), "move %d: decisions differ away from a CDF boundary (gap %.3g)" % (t, gap.max())
        decisions += int(live.sum())
        disagree += int(bad.sum())
    print("%s: %d decisions, %d differ from the f64 forward (all within 1e-5 of a CDF boundary)" % (mode, decisions, disagree))


def test_batch_of_one_rule(g2048):
    """With perturbed BatchNorm statistics the reference layout plays with its batch-of-one weights: the games of
    batchnorm="never", not those of "always"."""
    auto, never, always = (policy("random", "f32", bn) for bn in ("auto", "never", "always"))
    a, b, c = (play(p, 512, 400, "masked", 5) for p in (auto, never, always))
    assert_same(a, b, "auto vs never")
    assert not torch.equal(a["actions"], c["actions"])


def test_refill_and_placement_independence(g2048):
    pol = policy("random", "bf16")
    ref = play(pol, 2000, 2000, "masked", 8, base=3)
    for w in (1, 3):
        assert_same(ref, play(pol, 2000, 2000, "masked", 8, base=3, max_waves=w), "max_waves=%d" % w)
    pol = policy("reference", "f32")
    whole = play(pol, 4097, 600, "unmasked", 9, base=1 << 33)
    for w in (1, 3):
        assert_same(whole, play(pol, 4097, 600, "unmasked", 9, base=1 << 33, max_waves=w), "max_waves=%d" % w)
    assert_same(whole, play(pol, 4097, 600, "unmasked", 9, base=1 << 33), "two launches")
    lo = play(pol, 1000, 600, "unmasked", 9, base=1 << 33)
    hi = play(pol, 3097, 600, "unmasked", 9, base=(1 << 33) + 1000)
    for k in KEYS:
        assert torch.equal(torch.cat([lo[k], hi[k]]), whole[k]), "split at 1000: %s differs" % k


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_canaries_and_one_move(g2048, precision):
    from g2048 import _lib as L
    from g2048 import ops
    from g2048.vec import VecGame2048
    pol = policy("reference", precision)
    for n, cap in ((77, 1), (300, 50)):
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
        ws = torch.empty(L.lib().g2048_play_policy_workspace(n), dtype=torch.uint8, device=DEV)
        opts = L.POLICY_BF16 if precision == "bf16" else L.POLICY_F32
        L.call(torch.device(DEV), L.lib().g2048_play_policy_games, boards.data_ptr(), scores.data_ptr(),
               pol.actor.blob(1).data_ptr(), outs["moves"].data_ptr(), outs["valid"].data_ptr(), outs["invalid"].data_ptr(),
               outs["ms"].data_ptr(), outs["reward"].data_ptr(), outs["alive"].data_ptr(), outs["actions"].data_ptr(), cap, 3, 0, n,
               opts, 0, ws.data_ptr(), ws.numel(), L.stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()
        assert torch.equal(boards[n:], env.boards[n:]) and torch.equal(scores[n:], env.scores[n:])
        for k, v in outs.items():
            assert bool((v[n:] == (7 if k in ("alive", "actions") else -7)).all()), "%s written past n = %d" % (k, n)
        ref = play(pol, n, cap, "masked", 3)
        assert torch.equal(outs["moves"][:n], ref["moves"]) and torch.equal(outs["actions"][:n], ref["actions"])
        assert torch.equal(boards[:n], ref["boards"]) and torch.equal(outs["reward"][:n], ref["reward_sum"])
        if cap == 1:
            assert bool((outs["moves"][:n] == 1).all()) and bool((outs["alive"][:n] == 1).all())


def test_evaluate_policy_histories_and_drivers(g2048):
    pol = policy("reference", "f32")
    kw = dict(num_games=300, max_moves=2000, mode="masked", seed=17, game_id_base=40)
    res = g2048.evaluate_policy(pol, histories="best5", **kw)
    ref = g2048.evaluate_policy(pol, fused=False, **kw)
    for k in ("scores", "highest_tiles", "moves", "valid_moves", "invalid_moves", "milestones", "best_games", "unfinished",
              "episode_rewards"):
        assert res[k] == ref[k], k
    assert np.array_equal(res["final_boards"], ref["final_boards"])
    assert res["parameters"] == {"mode": "masked", "precision": "f32", "max_moves": 2000, "num_games": 300, "seed": 17}
    assert sorted(res["games"]) == sorted(res["best_games"])
    for i, game in res["games"].items():
        assert np.array_equal(game["board_history"][-1], res["final_boards"][i])
        assert game["scores_history"][-1] == res["scores"][i] and len(game["moveset"]) == res["moves"][i]
    print(res["summary"])
