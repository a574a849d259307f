"""g2048_ppo_collect (include/g2048_ppo_collect.h) and g2048.RolloutCollector(sampler="collect") on the MI355X: the one-launch
collector against the chain of entry points that were there before it, BIT FOR BIT. On the class level the yardstick is
RolloutCollector(sampler="fused", use_graph=False) with the same g2048.DevicePolicy; on the ops level ops.policy_forward +
ops.rollout_step per step, with ops.obs / ops.valid_moves for row 0 (`chain`). Compared: all T + 1 rows of the observations and
masks, actions, the stored probability (ops level) and its log (class level), rewards, flags, values, the next boards, the state
max codes, and the final boards and scores. Each case asserts, on the stepwise result, the condition that makes it a test; the
basics case holds the stepwise result against the CPU oracle too.

The networks are random-init modules of the reference's ActorNetwork / CriticNetwork layout with perturbed BatchNorm statistics,
as tests/test_gpu_policy.py builds them."""
import numpy as np
import pytest
import torch

import guard
from conftest import PKG, REPO  # noqa: F401
from test_gpu_qnet_collect import DEAD, DOM_EPISODE
from test_policy_host import RefLayout, perturb_bn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED, ID_BASE = 7, 5
FLAG_DONE, FLAG_VALID = 1, 2
_POLICIES = {}


def policy_of(precision="f32", critic=True):
    from g2048 import DevicePolicy
    key = (precision, critic)
    if key not in _POLICIES:
        torch.manual_seed(35)
        gen = torch.Generator().manual_seed(35)
        actor, value = perturb_bn(RefLayout(4), gen).to(DEV), perturb_bn(RefLayout(1), gen).to(DEV)
        _POLICIES[key] = DevicePolicy(actor, value if critic else None, precision=precision)
    return _POLICIES[key]


def collector(sampler, pol, n, T, prepare=None, **kw):
    from g2048 import RolloutCollector
    col = RolloutCollector(n, T, pol, device=DEV, seed=SEED, id_base=ID_BASE, sampler=sampler, use_graph=False, **kw)
    if prepare:
        prepare(col)
    return col


def snapshot(col, out):
    """Everything a collect() leaves behind, on the host: the dict's arrays, every row of the observations and masks, and the state."""
    torch.cuda.synchronize()
    r = {k: v for k, v in out.items() if v is not None and k not in ("obs", "valid_mask", "last_obs", "last_valid_mask")}
    r.update(obs=col._obs, masks=col._masks, flags=col.flags, boards=col.env.boards, scores=col.env.scores)
    for name in ("rewards64", "next_boards", "state_maxcode"):
        if getattr(col, name) is not None:
            r[name] = getattr(col, name)
    return {k: v.cpu().clone() for k, v in r.items()}


def assert_same(one_launch, stepwise, what=""):
    assert one_launch.keys() == stepwise.keys()
    for k in one_launch:
        assert guard.same_bits(one_launch[k], stepwise[k]), "%s differs between sampler='collect' and the stepwise chain %s" % (k, what)


def both(pol, n, T, collects=1, prepare=None, **kw):
    """(the stepwise results, one per collect, and its collector) after the one-launch results were found equal to them."""
    fused, one = collector("fused", pol, n, T, prepare, **kw), collector("collect", pol, n, T, prepare, **kw)
    results = []
    for c in range(collects):
        want, got = snapshot(fused, fused.collect()), snapshot(one, one.collect())
        assert_same(got, want, "(collect %d)" % c)
        results.append(want)
    assert one.env.t == fused.env.t == collects * T and int(one._counter) == collects * T and one.env_steps == fused.env_steps
    return results, fused, one


def chain(pol, boards0, scores0, steps, index0, reward_dtype=torch.float32, obs_dtype=torch.float32, counter=None):
    """`steps` steps from (boards0, scores0) with the older entry points, every array ops.ppo_collect can write."""
    from g2048 import ops
    n = boards0.shape[0]
    boards, scores, spare = boards0.clone(), scores0.clone(), torch.empty_like(boards0)
    z = lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype, device=DEV)      # noqa: E731
    r = dict(actions=z(steps, n), prob=z(steps, n, dtype=torch.float32), reward=z(steps, n, dtype=reward_dtype), flags=z(steps, n),
             value=z(steps, n, dtype=torch.float32), obs=z(steps + 1, n, 16, dtype=obs_dtype), mask=z(steps + 1, n),
             next_boards=z(steps, n, 16), state_maxcode=z(steps, n))
    ops.obs(boards, out=r["obs"][0])
    ops.valid_moves(boards, out=r["mask"][0])
    critic = pol.critic.blob(n) if pol.critic is not None else None
    for t in range(steps):
        out = ops.policy_forward(boards, pol.actor.blob(n), critic, pol.precision)
        probs = out[0] if critic is not None else out
        if critic is not None:
            r["value"][t].copy_(out[1].view(-1))
        ops.rollout_step(boards, probs, scores, SEED, index0 + t, ID_BASE, out=spare, actions=r["actions"][t], prob=r["prob"][t],
                         reward=r["reward"][t], flags=r["flags"][t], obs_next=r["obs"][t + 1], mask_next=r["mask"][t + 1],
                         next_boards=r["next_boards"][t], state_maxcode=r["state_maxcode"][t], auto_reset=True, step_counter=counter)
        boards, spare = spare, boards
    r.update(boards=boards, scores=scores)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in r.items()}


def start_state(n, seed=SEED):
    from g2048 import ops
    boards, scores = ops.reset(n, seed, 0, ID_BASE, device=DEV)
    return boards, scores


def fresh_codes(step_index, ids, oracle):
    """The board an episode that ended at `step_index` goes on from: oracle.env_reset of the two EPISODE-domain draws."""
    k0, k1 = oracle.rng_keys(SEED, DOM_EPISODE, step_index)
    tiles = np.stack([oracle.env_reset(oracle.rng_draw(k0, k1, i, 0), oracle.rng_draw(k0, k1, i, 1)) for i in ids])
    return np.where(tiles > 0, np.log2(np.maximum(tiles, 1)), 0).astype(np.uint8)


def test_basics_against_the_stepwise_collector_and_the_oracle(oracle):
    n, T = 33, 6
    dead = np.tile(DEAD, (2, 1))
    for a in range(4):           # on the CPU: every action leaves each of the eight boards finished
        _, _, _, fl = oracle.step_batch(dead, np.full(8, a, np.uint8), np.zeros(8, np.uint32), seed=SEED, step_index=0, id_base=ID_BASE)
        assert (fl & 1).all() and not (fl & 2).any()
    start = {}

    def prepare(col):
        col.env.boards[:8] = torch.from_numpy(dead).to(DEV)
        start["boards"] = col.env.boards.cpu().numpy().copy()

    pol = policy_of("f32")
    (r,), fused, _ = both(pol, n, T, prepare=prepare, shaping=True)
    assert r["rewards64"].dtype == torch.float64 and r["obs"].dtype == torch.float32 and "shaping" in r and "values" in r
    assert bool(r["values"].abs().sum() > 0) and tuple(r["obs"].shape) == (T + 1, n, 16)
    flags, masks, actions = r["flags"], r["masks"], r["actions"]
    assert bool((flags[0, :8] & FLAG_DONE).all()) and not bool((flags[0, :8] & FLAG_VALID).any()), "the eight dead boards end at t = 0"
    assert bool(((r["obs"][1, :8] > 0).sum(dim=1) == 2).all()), "and are played on from the fresh board: two tiles"
    assert bool((masks[0, :8] == 0).all()), "a mask of 0 occurred"
    # ... and was sampled among all four: the stored probability is the action's share of ALL four weights p + 1e-10
    p = pol(torch.from_numpy(dead).to(DEV))[0].cpu().double() + 1e-10
    share = (p / p.sum(dim=1, keepdim=True)).gather(1, actions[0, :8].long()[:, None]).squeeze(1)
    assert torch.allclose(r["log_prob"][0, :8].double().exp(), share, rtol=1e-5, atol=0) and len(set(actions[0, :8].tolist())) >= 2
    assert bool(((flags & FLAG_VALID) == 0).any()) and bool((masks != 15).any()), "an invalid move and a mask with fewer than four bits"
    # the stepwise yardstick itself against the CPU oracle: every transition, the resets and what is played on afterwards
    boards, scores = start["boards"], np.zeros(n, np.uint32)
    ids = range(ID_BASE, ID_BASE + n)
    for t in range(T):
        assert np.array_equal(r["obs"][t].numpy(), boards.astype(np.float32) / np.float32(15)), t
        assert np.array_equal(masks[t].numpy(), oracle.valid_moves_batch(boards)), t
        nxt, scores, reward, fl = oracle.step_batch(boards, actions[t].numpy(), scores, seed=SEED, step_index=t, id_base=ID_BASE)
        assert np.array_equal(r["next_boards"][t].numpy(), nxt) and np.array_equal(flags[t].numpy(), fl), t
        assert np.array_equal(r["rewards64"][t].numpy(), reward) and np.array_equal(r["rewards"][t].numpy(), reward.astype(np.float32)), t
        assert np.array_equal(r["state_maxcode"][t].numpy(), boards.max(axis=1)), t
        done = (fl & 1).astype(bool)
        boards = np.where(done[:, None], fresh_codes(t, ids, oracle), nxt)
        scores = np.where(done, 0, scores).astype(np.uint32)
    assert np.array_equal(r["boards"].numpy(), boards) and np.array_equal(r["scores"].numpy().astype(np.uint32), scores)
    assert np.array_equal(r["obs"][T].numpy(), boards.astype(np.float32) / np.float32(15))
    fused.check()


EDGES = [("f32", n, T) for n in (1, 31, 32, 33) for T in (1, 5)] + [("bf16", n, T) for n in (1, 63, 64, 65) for T in (1, 5)] + \
        [("f32", 300, 3), ("bf16", 300, 3)]


@pytest.mark.parametrize("precision,n,T", EDGES, ids=["%s_n%d_T%d" % e for e in EDGES])
def test_wavefront_edges_and_several_blocks(precision, n, T):
    pol = policy_of(precision)
    (r,), _, _ = both(pol, n, T)
    assert tuple(r["actions"].shape) == (T, n) and tuple(r["obs"].shape) == (T + 1, n, 16) and tuple(r["boards"].shape) == (n, 16)
    assert bool(r["values"].abs().sum() > 0) and bool((r["log_prob"] <= 0).all())
    if n == 1:      # the reference's rule for a batch of one row: the blob without BatchNorm
        assert pol.actor.blob(1) is pol.actor.packed["off"] and pol.actor.blob(2) is pol.actor.packed["on"]
        assert not torch.equal(pol.actor.packed["off"], pol.actor.packed["on"])
    if precision == "bf16" and n > 1:
        start = torch.round(r["obs"][0] * 15).to(torch.uint8).to(DEV)
        assert not torch.equal(pol(start)[0], policy_of("f32")(start)[0]), "the bf16 blob gave the f32 network's probabilities"


@pytest.mark.parametrize("option", ["actor_only", "obs_f16", "obs_bf16"])
def test_options_of_the_class(option):
    pol = policy_of("f32", critic=option != "actor_only")
    dtype = {"obs_f16": torch.float16, "obs_bf16": torch.bfloat16}.get(option, torch.float32)
    (r,), _, one = both(pol, 33, 3, obs_dtype=dtype)
    assert r["obs"].dtype == dtype and r["rewards"].dtype == torch.float32 and "rewards64" not in r, "the f32 reward"
    if option == "actor_only":
        assert pol.critic is None and not bool(r["values"].any()), "no critic: the values stay as they were"
    else:
        assert bool((r["obs"].float() != torch.round(r["obs"].float() * 15) / 15).any()), "the 16-bit observations are rounded once more"


def test_absent_outputs_and_the_stored_probability_on_the_ops_level():
    from g2048 import ops
    n, steps = 33, 3
    boards0, scores0 = start_state(n)
    for pol in (policy_of("f32"), policy_of("f32", critic=False)):
        want = chain(pol, boards0, scores0, steps, 0)
        critic = pol.critic.blob(n) if pol.critic is not None else None
        # everything given
        boards, scores = boards0.clone(), scores0.clone()
        obs = torch.zeros((steps + 1, n, 16), device=DEV)
        mask, nb, sm = [torch.zeros(s, dtype=torch.uint8, device=DEV) for s in ((steps + 1, n), (steps, n, 16), (steps, n))]
        actions, prob, reward, flags, value = ops.ppo_collect(boards, scores, pol.actor.blob(n), critic, steps, "f32", SEED, 0, ID_BASE,
                                                              obs=obs, mask=mask, next_boards=nb, state_maxcode=sm)
        got = dict(actions=actions, prob=prob, reward=reward, flags=flags, obs=obs, mask=mask, next_boards=nb, state_maxcode=sm,
                   boards=boards, scores=scores)
        assert (value is None) == (critic is None)
        if critic is not None:
            got["value"] = value
        torch.cuda.synchronize()
        for k, v in got.items():
            assert guard.same_bits(v, want[k]), k
        assert bool((want["prob"] > 0).all()) and bool((want["prob"] <= 1).all()) and bool((want["prob"] < 1).any()), "a probability, not its log"
        # obs, mask, next_boards and state_maxcode absent: the rest is the same
        boards, scores = boards0.clone(), scores0.clone()
        bare = ops.ppo_collect(boards, scores, pol.actor.blob(n), critic, steps, "f32", SEED, 0, ID_BASE)
        torch.cuda.synchronize()
        for k, v in zip(("actions", "prob", "reward", "flags"), bare):
            assert guard.same_bits(v, want[k]), k
        assert guard.same_bits(boards, want["boards"]) and guard.same_bits(scores, want["scores"])


def test_the_step_index_with_and_without_the_device_counter():
    from g2048 import ops
    n, steps = 33, 2
    pol = policy_of("f32")
    boards0, scores0 = start_state(n)
    want = chain(pol, boards0, scores0, steps, 3)
    assert not guard.same_bits(want["actions"], chain(pol, boards0, scores0, steps, 0)["actions"]), "the step index decides nothing here"
    counter = torch.full((1,), 2, dtype=torch.int64, device=DEV)
    for index0, ctr in ((3, None), (1, counter)):
        boards, scores = boards0.clone(), scores0.clone()
        obs = torch.zeros((steps + 1, n, 16), device=DEV)
        actions, prob, reward, flags, value = ops.ppo_collect(boards, scores, pol.actor.blob(n), pol.critic.blob(n), steps, "f32", SEED,
                                                              index0, ID_BASE, obs=obs, step_counter=ctr)
        torch.cuda.synchronize()
        for k, v in dict(actions=actions, prob=prob, reward=reward, flags=flags, value=value, obs=obs, boards=boards).items():
            assert guard.same_bits(v, want[k]), (k, index0)
    assert int(counter) == 2, "the call advanced the counter it only reads"


def test_two_collects_in_a_row_with_shaping_and_a_minibatch():
    (first, second), fused, one = both(policy_of("f32"), 33, 4, collects=2, shaping=True)
    assert guard.same_bits(second["obs"][0], first["obs"][4]) and guard.same_bits(second["masks"][0], first["masks"][4]), "row T carries over"
    assert not guard.same_bits(second["actions"], first["actions"]) and bool(torch.isfinite(second["shaping"]).all())
    a, b = one.sample(64, want_indices=True), fused.sample(64, want_indices=True)
    torch.cuda.synchronize()
    assert a.keys() == b.keys() and len(set(a["indices"].tolist())) == 64
    for k in a:
        assert guard.same_bits(a[k], b[k]), k
    one.check()


def test_one_captured_graph_replays_as_the_next_collects():
    """The captured collect() is one g2048_ppo_collect kernel followed, on the same stream, by torch's elementwise kernels (the
    counter's add, the log, the dict's views of the flags): one chain, no parallel branches."""
    n, T = 64, 2
    pol = policy_of("bf16")
    eager = collector("fused", pol, n, T)
    collector("collect", pol, n, T).collect()          # the library is loaded and torch's kernels are warm before the capture
    one = collector("collect", pol, n, T)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = one.collect()
    for c in range(2):
        graph.replay()
        got, want = snapshot(one, out), snapshot(eager, eager.collect())
        assert_same(got, want, "(replay %d)" % c)
    assert int(one._counter) == 2 * T


def test_guard_bands_round_everything_the_call_writes():
    from g2048 import ops
    n, steps = 33, 3
    pol = policy_of("f32")
    boards0, scores0 = start_state(n)
    counter0 = torch.full((1,), 2, dtype=torch.int64)

    def call(S):
        boards, scores = S.inp("boards", boards0.cpu(), align=16), S.inp("scores", scores0.cpu(), align=4)
        actor, critic = S.inp("actor", pol.actor.blob(n).cpu(), align=16), S.inp("critic", pol.critic.blob(n).cpu(), align=16)
        counter = S.inp("counter", counter0, align=8)
        out = dict(actions=S.out("actions", steps, (n,)), prob=S.out("prob", steps, (n,), torch.float32),
                   reward=S.out("reward", steps, (n,), torch.float64), flags=S.out("flags", steps, (n,)),
                   value=S.out("value", steps, (n,), torch.float32), obs=S.out("obs", steps + 1, (n, 16), torch.float32, align=16),
                   mask=S.out("mask", steps + 1, (n,)), next_boards=S.out("next_boards", steps, (n, 16), align=16),
                   state_maxcode=S.out("state_maxcode", steps, (n,)))
        ops.ppo_collect(boards, scores, actor, critic, steps, "f32", SEED, 1, ID_BASE, step_counter=counter, **out)
        return dict(out, boards=boards, scores=scores, counter=counter)

    out = guard.twice(DEV, call)
    want = chain(pol, boards0, scores0, steps, 3, reward_dtype=torch.float64)
    for k, v in want.items():
        assert guard.same_bits(out[k], v), k
    assert int(out["counter"]) == 2 and not guard.same_bits(out["boards"], boards0)


def test_the_sampler_needs_a_device_policy():
    from g2048 import RolloutCollector

    class Stock(torch.nn.Module):
        def forward(self, obs):
            return torch.full((obs.shape[0], 4), 0.25, device=obs.device)

    with pytest.raises(ValueError, match="needs a g2048.DevicePolicy"):
        RolloutCollector(8, 2, Stock(), device=DEV, sampler="collect")
    with pytest.raises(ValueError, match="sampler must be"):
        RolloutCollector(8, 2, policy_of("f32"), device=DEV, sampler="one_launch")
