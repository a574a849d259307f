"""g2048_play_tpolicy_games on the MI355X: the fused kernel against the unfused loop of existing launches (every output, bit
for bit), the recorded decisions against the CPU oracle and against tpolicy.forward_reference in float64, independence of the
block count and of the id split, canaries past n, and evaluate_policy with a DeviceTransformerPolicy.

The networks carry the hash-derived weights of tests/tpolicy_weights.py: the fixture's (dim_ff 2048, 2 layers), a small one
(dim_ff 32, 1 layer) and the bench shape (dim_ff 128, 2 layers)."""
import numpy as np
import pytest
import torch

import tpolicy_weights as tw
from test_tpolicy_host import RefSpelling

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("boards", "scores", "moves", "valid_moves", "invalid_moves", "milestone_move", "alive", "reward_sum", "actions")
SHAPES = {"fixture": (2048, 2), "small": (32, 1), "bench": (128, 2)}
_MODELS, _POLICIES = {}, {}


@pytest.fixture(scope="module")
def g2048():
    import __graft_entry__ as ge
    ge.ensure_built()
    return ge.import_package()


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


def forward_of(pol):
    from g2048 import ops
    return lambda boards, probs: ops.tpolicy_forward(boards, pol.packed, pol.dim_ff, pol.n_layers, pol.precision, probs=probs,
                                                     want_value=False)


def play(pol, n, max_moves, mode, seed, base=0, fused=True, max_blocks=0):
    from g2048 import ops
    from g2048.evaluate import _play_policy_stepwise
    from g2048.vec import VecGame2048
    env = VecGame2048(n, device=torch.device(DEV), seed=seed, id_base=base)
    start = env.boards.clone()
    if fused:
        r = ops.play_tpolicy_games(env.boards, env.scores, pol.packed, pol.dim_ff, pol.n_layers, pol.precision, max_moves, mode, seed,
                                   base, want_rewards=True, want_actions=True, max_blocks=max_blocks)
    else:
        r = _play_policy_stepwise(env, pol.packed, pol.precision, max_moves, mode, seed, base, forward=forward_of(pol))
    torch.cuda.synchronize()
    r.update(boards=env.boards, scores=env.scores, start=start)
    return r


def assert_same(a, b, what):
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), "%s: %s differ" % (what, k)


@pytest.mark.parametrize("network", ["fixture", "small"])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ["masked", "unmasked", "greedy"])
def test_fused_equals_unfused(g2048, mode, precision, network):
    pol = policy(network, precision)
    for n, cap in ((1, 2000), (15, 2000), (17, 2000), (4097, 2000), (4097, 37)):
        seed = 1000 + n + cap
        a = play(pol, n, cap, mode, seed, fused=False)
        b = play(pol, n, cap, mode, seed, fused=True)
        assert_same(a, b, "%s %s %s n=%d cap=%d" % (mode, precision, network, n, cap))
        if cap == 37:
            assert int(b["alive"].sum()) > 0 and int((b["moves"] == 37).sum()) >= int(b["alive"].sum())
        assert int(b["moves"].min()) >= 1 and bool((b["valid_moves"] + b["invalid_moves"] == b["moves"]).all())
        assert bool((b["moves"] <= cap).all()) and bool(((b["moves"] == cap) | (b["alive"] == 0)).all())


def test_fused_equals_unfused_65536(g2048):
    pol = policy("bench", "f32")
    a = play(pol, 65536, 2000, "masked", 77, base=12345, fused=False)
    b = play(pol, 65536, 2000, "masked", 77, base=12345, fused=True)
    assert_same(a, b, "65536 games")
    m = b["moves"].double()
    print("hash weights dim_ff 128, masked, f32: mean game %.1f moves, longest %d" % (m.mean().item(), int(m.max().item())))


def replay_and_forward(pol, r, seed):
    """Every pre-move board of every game (g2048_replay_games) and the policy's probabilities for it (g2048_tpolicy_forward)."""
    from g2048 import ops
    longest = int(r["moves"].max().item())
    bh, sh, fh = ops.replay_games(r["start"], r["actions"], r["moves"], seed, longest=longest)
    k = bh.shape[0]
    probs = ops.tpolicy_forward(bh[:, :longest].reshape(k * longest, 16).contiguous(), pol.packed, pol.dim_ff, pol.n_layers,
                                pol.precision, want_value=False)
    torch.cuda.synchronize()
    return bh.cpu().numpy(), sh.cpu().numpy(), probs.view(k, longest, 4).cpu().numpy(), longest


@pytest.mark.parametrize("mode", ["masked", "unmasked"])
def test_decisions_and_moves_against_the_oracle(g2048, oracle, mode):
    """256 complete games: replaying the recorded actions with the oracle's env step gives g2048_replay_games' histories and
    the kernel's final state, counters, milestones and f64 reward sums; the oracle's sampler on the device forward's
    probabilities of every pre-move board gives the recorded action of every move."""
    pol = policy("fixture", "f32")
    n, seed = 256, 4242
    r = play(pol, n, 2000, mode, seed)
    bh, sh, probs, longest = replay_and_forward(pol, r, seed)
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
    fin = np.arange(n)
    assert np.array_equal(b, bh[fin, moves]) and np.array_equal(sc, sh[fin, moves].astype(np.uint32))
    assert np.array_equal(b, r["boards"].cpu().numpy()) and np.array_equal(sc, r["scores"].cpu().numpy().astype(np.uint32))
    assert np.array_equal(rsum, r["reward_sum"].cpu().numpy()), "f64 reward sums differ"
    assert np.array_equal(valid, r["valid_moves"].cpu().numpy()) and np.array_equal(ms, r["milestone_move"].cpu().numpy())
    assert np.array_equal(moves - valid, r["invalid_moves"].cpu().numpy())
    assert bool((acts[np.arange(acts.shape[1])[None, :] >= moves[:, None]] == 0xFF).all())


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
    bh, _, _, longest = replay_and_forward(pol, r, seed)
    moves = r["moves"].cpu().numpy()
    acts = r["actions"].cpu().numpy()
    game, move = np.nonzero(np.arange(longest)[None, :] < moves[:, None])           # every decision (game, move)
    boards = torch.from_numpy(bh[game, move])
    p64 = torch.cat([tpolicy.forward_reference(parsed, boards[i:i + 4096])[0] for i in range(0, len(boards), 4096)]).numpy()
    mask = oracle.valid_moves_batch(bh[game, move]) if mode == "masked" else np.full(len(game), 15, np.uint8)
    keys = [oracle.rng_keys(seed, oracle.DOM_POLICY, t) for t in range(longest)]
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
    print("%s: %d decisions, %d differ from the f64 forward (%.3g of all; largest gap to a CDF boundary %.3g)" % (
        mode, len(game), int(bad.sum()), bad.mean(), gap.max() if bad.any() else 0.0))
    assert (gap <= GAP_BOUND).all(), "decisions differ away from a CDF boundary (gap %.3g)" % gap.max()
    assert bad.sum() <= RATE_BOUND * len(game)


def test_refill_and_placement_independence(g2048):
    pol = policy("small", "bf16")
    ref = play(pol, 2000, 2000, "masked", 8, base=3)
    for blocks in (1, 3):
        assert_same(ref, play(pol, 2000, 2000, "masked", 8, base=3, max_blocks=blocks), "max_blocks=%d" % blocks)
    pol = policy("fixture", "f32")
    ref = play(pol, 2000, 2000, "masked", 8, base=3)
    assert_same(ref, play(pol, 2000, 2000, "masked", 8, base=3, max_blocks=3), "fixture, max_blocks=3")
    whole = play(pol, 2000, 2000, "unmasked", 9, base=1 << 33)
    assert_same(whole, play(pol, 2000, 2000, "unmasked", 9, base=1 << 33), "two launches")
    lo = play(pol, 1000, 2000, "unmasked", 9, base=1 << 33)
    hi = play(pol, 1000, 2000, "unmasked", 9, base=(1 << 33) + 1000)
    for k in KEYS:
        assert torch.equal(torch.cat([lo[k], hi[k]]), whole[k]), "split at 1000: %s differs" % k


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_canaries_and_one_move(g2048, precision):
    from g2048 import _lib as L
    from g2048 import ops
    from g2048.vec import VecGame2048
    pol = policy("fixture", precision)
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
            ws = torch.empty(L.lib().g2048_play_tpolicy_workspace(n), dtype=torch.uint8, device=DEV)
            opts = L.POLICY_BF16 if precision == "bf16" else L.POLICY_F32
            L.call(torch.device(DEV), L.lib().g2048_play_tpolicy_games, boards.data_ptr(), scores.data_ptr(), pol.packed.data_ptr(),
                   pol.dim_ff, pol.n_layers, outs["moves"].data_ptr(), outs["valid"].data_ptr(), outs["invalid"].data_ptr(),
                   outs["ms"].data_ptr(), outs["reward"].data_ptr(), outs["alive"].data_ptr(), outs["actions"].data_ptr(), cap, 3, 0, n,
                   opts, 0, ws.data_ptr(), ws.numel(), L.stream_ptr(torch.device(DEV)))
            torch.cuda.synchronize()
            assert torch.equal(boards[n:], env.boards[n:]) and torch.equal(scores[n:], env.scores[n:])
            for k, v in outs.items():
                assert bool((v[n:] == (7 if k in ("alive", "actions") else -7)).all()), "%s written past n = %d" % (k, n)
            ref = play(pol, n, cap, "masked", 3)
            assert torch.equal(outs["moves"][:n], ref["moves"]) and torch.equal(outs["actions"][:n], ref["actions"])
            assert torch.equal(boards[:n], ref["boards"]) and torch.equal(outs["reward"][:n], ref["reward_sum"])
            assert torch.equal(outs["ms"][:n], ref["milestone_move"]) and torch.equal(outs["alive"][:n], ref["alive"])
            if cap == 1:
                assert bool((outs["moves"][:n] == 1).all()) and bool((outs["alive"][:n] == 1).all())
    with pytest.raises(ValueError, match="blob of"):
        env = VecGame2048(4, device=torch.device(DEV), seed=3)
        ops.play_tpolicy_games(env.boards, env.scores, pol.packed[:-16].contiguous(), pol.dim_ff, pol.n_layers, precision)


def test_evaluate_policy_histories_drivers_and_refresh(g2048):
    import copy
    from g2048 import DeviceTransformerPolicy
    pol = DeviceTransformerPolicy(copy.deepcopy(hash_model("fixture")).float().to(DEV), precision="f32")
    kw = dict(num_games=300, max_moves=2000, mode="masked", seed=17, game_id_base=40)
    res = g2048.evaluate_policy(pol, histories="best5", **kw)
    ref = g2048.evaluate_policy(pol, fused=False, **kw)
    for k in ("scores", "highest_tiles", "moves", "valid_moves", "invalid_moves", "milestones", "milestones_by_game", "best_games",
              "best_score", "best_game_idx", "unfinished", "total_moves", "total_expansions", "episode_rewards", "parameters"):
        assert res[k] == ref[k], k
    assert set(res) - {"games"} == set(ref)
    assert np.array_equal(res["final_boards"], ref["final_boards"]) and np.array_equal(res["best_board"], ref["best_board"])
    assert res["parameters"] == {"mode": "masked", "precision": "f32", "max_moves": 2000, "num_games": 300, "seed": 17}
    assert sorted(res["games"]) == sorted(res["best_games"])
    for i, game in res["games"].items():
        assert np.array_equal(game["board_history"][-1], res["final_boards"][i])
        assert game["scores_history"][-1] == res["scores"][i] and len(game["moveset"]) == res["moves"][i]
    print(res["summary"])
    with torch.no_grad():
        pol.model.actor.weight.mul_(-1.0)
    assert g2048.evaluate_policy(pol, **kw)["moves"] == res["moves"]             # the packed weights are what plays
    pol.refresh()
    assert g2048.evaluate_policy(pol, **kw)["moves"] != res["moves"]
