"""g2048_tpolicy_collect (include/g2048_tpolicy_collect.h) and g2048.RolloutCollector(sampler="collect") with a
g2048.DeviceTransformerPolicy on the MI355X: the one-launch collector against the chain of entry points that were there before
it, BIT FOR BIT. On the class level the yardstick is RolloutCollector(sampler="fused", use_graph=False) with the same policy; on
the ops level ops.tpolicy_forward + ops.rollout_step per step, with ops.obs / ops.valid_moves for row 0 (`chain`). Compared: all
T + 1 rows of the observations and masks, actions, the stored probability (ops level) and its log (class level), rewards, flags,
values, the next boards, the state max codes, the final boards and scores, env.t and the counter. Each case asserts, on the
stepwise result, the condition that makes it a test; the basics case holds the stepwise result against the CPU oracle too.

The networks carry the hash-derived weights of tests/tpolicy_weights.py, as tests/test_gpu_tpolicy_play.py builds them: `small`
(dim_ff 32, 1 layer) unless said otherwise."""
import copy

import numpy as np
import pytest
import torch

import guard
from conftest import PKG, REPO  # noqa: F401
from test_gpu_qnet_collect import DEAD, DOM_EPISODE
from test_gpu_tpolicy_play import SHAPES, hash_model, policy

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED, ID_BASE = 7, 5
FLAG_DONE, FLAG_VALID = 1, 2


def own_policy(network, precision):
    """A policy of its own module, for the test that changes the weights (`policy` caches one per network and precision)."""
    from g2048 import DeviceTransformerPolicy
    return DeviceTransformerPolicy(copy.deepcopy(hash_model(network)).float().to(DEV), precision=precision)


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
    """`steps` steps from (boards0, scores0) with the older entry points, every array ops.tpolicy_collect can write."""
    from g2048 import ops
    n = boards0.shape[0]
    boards, scores, spare = boards0.clone(), scores0.clone(), torch.empty_like(boards0)
    z = lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype, device=DEV)      # noqa: E731
    r = dict(actions=z(steps, n), prob=z(steps, n, dtype=torch.float32), reward=z(steps, n, dtype=reward_dtype), flags=z(steps, n),
             value=z(steps, n, dtype=torch.float32), obs=z(steps + 1, n, 16, dtype=obs_dtype), mask=z(steps + 1, n),
             next_boards=z(steps, n, 16), state_maxcode=z(steps, n))
    ops.obs(boards, out=r["obs"][0])
    ops.valid_moves(boards, out=r["mask"][0])
    for t in range(steps):
        probs, value = ops.tpolicy_forward(boards, pol.packed, pol.dim_ff, pol.n_layers, pol.precision)
        r["value"][t].copy_(value.view(-1))
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


def collect_op(pol, boards, scores, steps, index0=0, **kw):
    from g2048 import ops
    return ops.tpolicy_collect(boards, scores, pol.packed, pol.dim_ff, pol.n_layers, steps, pol.precision, SEED, index0, ID_BASE, **kw)


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

    pol = policy("small", "f32")
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
    assert torch.allclose(r["log_prob"][0, :8].double().exp(), share, rtol=1e-5, atol=0)
    # masks with fewer than four bits: whatever the policy, start boards 11, 12 and 13 of (seed 7, id base 5) have 12, 7 and 14
    assert masks[0, 11:14].tolist() == [12, 7, 14] and bool((masks != 15).any())
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


# a wavefront owns 4 boards, a block 16: one live slot, a block one short, a full one, one env in a second block whose wavefronts
# 1..3 have none, and four blocks of which the last holds 2 envs
EDGES = [(p, n, T) for p in ("f32", "bf16") for n in (1, 15, 16, 17, 50) for T in (1, 5)]


@pytest.mark.parametrize("precision,n,T", EDGES, ids=["%s_n%d_T%d" % e for e in EDGES])
def test_block_and_wavefront_edges(precision, n, T):
    pol = policy("small", precision)
    (r,), _, _ = both(pol, n, T)
    assert tuple(r["actions"].shape) == (T, n) and tuple(r["obs"].shape) == (T + 1, n, 16) and tuple(r["boards"].shape) == (n, 16)
    assert bool(r["values"].abs().sum() > 0) and bool((r["log_prob"] <= 0).all())
    if precision == "bf16":
        start = torch.round(r["obs"][0] * 15).to(torch.uint8).to(DEV)
        assert not torch.equal(pol(start)[0], policy("small", "f32")(start)[0]), "the bf16 blob gave the f32 network's probabilities"


SHAPED = [(w, p) for w in ("odd", "fixture") for p in ("f32", "bf16")]


@pytest.mark.parametrize("network,precision", SHAPED, ids=["%s-%s" % c for c in SHAPED])
def test_network_shapes_inside_the_step_loop(network, precision):
    """dim_ff 96 with 3 layers (an odd number of 32-feature slices, a third layer's offsets) and the fixture's 2,048 with 2."""
    pol = policy(network, precision)
    assert (pol.dim_ff, pol.n_layers) == SHAPES[network]
    (r,), _, _ = both(pol, 17, 2)
    assert bool(r["values"].abs().sum() > 0) and not guard.same_bits(r["values"][0], r["values"][1])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["obs_f16", "obs_bf16"])
def test_sixteen_bit_observations(dtype):
    (r,), _, one = both(policy("small", "f32"), 33, 3, obs_dtype=dtype)
    assert r["obs"].dtype == dtype and r["rewards"].dtype == torch.float32 and "rewards64" not in r, "the f32 reward"
    assert bool((r["obs"].float() != torch.round(r["obs"].float() * 15) / 15).any()), "the 16-bit observations are rounded once more"


def test_absent_outputs_values_left_alone_and_the_stored_probability_on_the_ops_level():
    n, steps = 33, 3
    pol = policy("small", "f32")
    boards0, scores0 = start_state(n)
    want = chain(pol, boards0, scores0, steps, 0)
    # everything given
    boards, scores = boards0.clone(), scores0.clone()
    obs = torch.zeros((steps + 1, n, 16), device=DEV)
    mask, nb, sm = [torch.zeros(s, dtype=torch.uint8, device=DEV) for s in ((steps + 1, n), (steps, n, 16), (steps, n))]
    actions, prob, reward, flags, value = collect_op(pol, boards, scores, steps, obs=obs, mask=mask, next_boards=nb, state_maxcode=sm)
    got = dict(actions=actions, prob=prob, reward=reward, flags=flags, value=value, obs=obs, mask=mask, next_boards=nb, state_maxcode=sm,
               boards=boards, scores=scores)
    torch.cuda.synchronize()
    for k, v in got.items():
        assert guard.same_bits(v, want[k]), k
    assert bool((want["prob"] > 0).all()) and bool((want["prob"] <= 1).all()) and bool((want["prob"] < 1).any()), "a probability, not its log"
    # obs, mask, next_boards and state_maxcode absent, and no values wanted: the rest is the same and no value tensor comes back
    boards, scores = boards0.clone(), scores0.clone()
    bare = collect_op(pol, boards, scores, steps, want_value=False)
    torch.cuda.synchronize()
    assert bare[4] is None
    for k, v in zip(("actions", "prob", "reward", "flags"), bare):
        assert guard.same_bits(v, want[k]), k
    assert guard.same_bits(boards, want["boards"]) and guard.same_bits(scores, want["scores"])
    # want_value=False with the default outputs only: a value tensor that is given is written all the same
    boards, scores = boards0.clone(), scores0.clone()
    kept = torch.full((steps, n), 3.5, device=DEV)
    assert collect_op(pol, boards, scores, steps, want_value=False, value=kept)[4] is kept
    torch.cuda.synchronize()
    assert guard.same_bits(kept, want["value"])


def test_the_step_index_with_and_without_the_device_counter():
    n, steps = 33, 2
    pol = policy("small", "f32")
    boards0, scores0 = start_state(n)
    want = chain(pol, boards0, scores0, steps, 3)
    assert not guard.same_bits(want["actions"], chain(pol, boards0, scores0, steps, 0)["actions"]), "the step index decides nothing here"
    counter = torch.full((1,), 2, dtype=torch.int64, device=DEV)
    for index0, ctr in ((3, None), (1, counter)):
        boards, scores = boards0.clone(), scores0.clone()
        obs = torch.zeros((steps + 1, n, 16), device=DEV)
        actions, prob, reward, flags, value = collect_op(pol, boards, scores, steps, index0, obs=obs, step_counter=ctr)
        torch.cuda.synchronize()
        for k, v in dict(actions=actions, prob=prob, reward=reward, flags=flags, value=value, obs=obs, boards=boards).items():
            assert guard.same_bits(v, want[k]), (k, index0)
    assert int(counter) == 2, "the call advanced the counter it only reads"


def test_two_collects_in_a_row_with_shaping_and_minibatches_as_floats_and_as_boards():
    T, n = 4, 33
    (first, second), fused, one = both(policy("small", "f32"), n, T, collects=2, shaping=True)
    assert guard.same_bits(second["obs"][0], first["obs"][T]) and guard.same_bits(second["masks"][0], first["masks"][T]), "row T carries over"
    assert not guard.same_bits(second["actions"], first["actions"]) and bool(torch.isfinite(second["shaping"]).all())
    a, b = one.sample(64, want_indices=True), fused.sample(64, want_indices=True)
    torch.cuda.synchronize()
    assert a.keys() == b.keys() and len(set(a["indices"].tolist())) == 64
    for k in a:
        assert guard.same_bits(a[k], b[k]), k
    # as packed boards, what DeviceTransformerPolicy.update() takes: the boards the sampled rows were encoded from
    c = one.sample(64, want_indices=True, as_boards=True)
    torch.cuda.synchronize()
    assert c.keys() == a.keys() and c["states"].dtype == c["next_states"].dtype == torch.uint8 and tuple(c["states"].shape) == (64, 16)
    idx = c["indices"].cpu()
    assert len(set(idx.tolist())) == 64 and not torch.equal(idx, a["indices"].cpu()), "the next draw, not the last one again"
    assert torch.equal(c["next_states"].cpu(), second["next_boards"].view(-1, 16)[idx])
    acted_in = torch.round(second["obs"][:T].reshape(-1, 16) * 15).to(torch.uint8)     # float32 observations: code / 15 exactly
    assert torch.equal(acted_in[:n], first["boards"]), "row 0 = the boards the first collect ended on"
    went_on = (second["flags"].view(-1)[:-n] & FLAG_DONE) == 0                          # rows 1..: the next board where no episode ended
    assert torch.equal(acted_in[n:][went_on], second["next_boards"].view(-1, 16)[:-n][went_on]) and bool(went_on.any())
    assert torch.equal(c["states"].cpu(), acted_in[idx])
    for k in ("actions", "old_log_probs", "rewards", "dones"):
        assert c[k].dtype == a[k].dtype and c[k].shape == a[k].shape
    with pytest.raises(ValueError, match="as_boards=False"):
        one.sample(64, out=a, as_boards=True)
    one.check()


def test_weights_changed_in_place_act_in_the_next_collect():
    n, T = 17, 3
    pol = own_policy("small", "f32")
    fused, one, old = collector("fused", pol, n, T), collector("collect", pol, n, T), collector("collect", pol, n, T)
    assert_same(snapshot(one, one.collect()), snapshot(fused, fused.collect()), "(before the change)")
    old.collect()
    stale = snapshot(old, old.collect())            # the second collect with the OLD weights, from the same state
    with torch.no_grad():
        for p in pol.model.parameters():
            p.add_(0.05 * torch.sin(torch.arange(p.numel(), device=DEV, dtype=torch.float32)).view(p.shape))
    before = pol.packed.clone()
    pol.refresh()
    assert not torch.equal(pol.packed, before), "refresh() left the blob as it was"
    got, want = snapshot(one, one.collect()), snapshot(fused, fused.collect())
    assert_same(got, want, "(after refresh())")
    assert guard.same_bits(got["obs"][0], stale["obs"][0]), "the same state ..."
    assert not guard.same_bits(got["log_prob"], stale["log_prob"]) and not guard.same_bits(got["values"], stale["values"]), "... other weights"


def test_one_captured_graph_replays_as_the_next_collects():
    """The captured collect() is one g2048_tpolicy_collect kernel followed, on the same stream, by torch's elementwise kernels (the
    counter's add, the log, the dict's views of the flags): one chain, no parallel branches."""
    n, T = 16, 2
    pol = policy("small", "bf16")
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
    pol = policy("small", "f32")
    boards0, scores0 = start_state(n)
    counter0 = torch.full((1,), 2, dtype=torch.int64)

    def call(S):
        boards, scores = S.inp("boards", boards0.cpu(), align=16), S.inp("scores", scores0.cpu(), align=4)
        packed, counter = S.inp("packed", pol.packed.cpu(), align=16), S.inp("counter", counter0, align=8)
        out = dict(actions=S.out("actions", steps, (n,)), prob=S.out("prob", steps, (n,), torch.float32),
                   reward=S.out("reward", steps, (n,), torch.float64), flags=S.out("flags", steps, (n,)),
                   value=S.out("value", steps, (n,), torch.float32), obs=S.out("obs", steps + 1, (n, 16), torch.float32, align=16),
                   mask=S.out("mask", steps + 1, (n,)), next_boards=S.out("next_boards", steps, (n, 16), align=16),
                   state_maxcode=S.out("state_maxcode", steps, (n,)))
        ops.tpolicy_collect(boards, scores, packed, pol.dim_ff, pol.n_layers, steps, "f32", SEED, 1, ID_BASE, step_counter=counter, **out)
        return dict(out, boards=boards, scores=scores, counter=counter)

    out = guard.twice(DEV, call)
    want = chain(pol, boards0, scores0, steps, 3, reward_dtype=torch.float64)
    for k, v in want.items():
        assert guard.same_bits(out[k], v), k
    assert int(out["counter"]) == 2 and not guard.same_bits(out["boards"], boards0)


def test_the_sampler_takes_both_device_policies_and_nothing_else():
    from g2048 import RolloutCollector

    class Stock(torch.nn.Module):
        def forward(self, obs):
            return torch.full((obs.shape[0], 4), 0.25, device=obs.device)

    with pytest.raises(ValueError, match="needs a g2048.DevicePolicy"):
        RolloutCollector(8, 2, Stock(), sampler="collect")
    with pytest.raises(ValueError, match="sampler must be"):
        RolloutCollector(8, 2, policy("small", "f32"), device=DEV, sampler="one_launch")
    col = RolloutCollector(8, 2, policy("small", "f32"), device=DEV, sampler="collect")
    assert col.sampler == "collect" and not col.use_graph and tuple(col.collect()["actions"].shape) == (2, 8)
