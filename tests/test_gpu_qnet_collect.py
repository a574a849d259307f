"""g2048_qnet_collect (include/g2048_collect.h) and g2048.DQNCollector on the MI355X: the one-launch collector against
collect(fused=False), the same function made of the entry points that were there before it (net.act / net.act_beam, ops.step
without and with auto-reset, buffer.push), BIT FOR BIT: all six ring arrays over the whole capacity, size, head, the flags stream
and the final boards, scores and move counts. Each case asserts, on the stepwise result, the condition that makes it a test.
The stepwise path itself is held against the CPU oracle where a case says so.

The networks are random-init modules of the reference's structure (tests/test_qnet_host.py::RefSpelling), dim_ff 32 and one
layer unless a case says otherwise."""
import numpy as np
import pytest
import torch

import guard
from conftest import PKG, REPO  # noqa: F401
from test_policy_host import distinct_layers, random_boards
from test_qnet_host import RefSpelling

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED, ID_BASE = 7, 5
DOM_EPISODE = 6
RING = ("states", "next_states", "actions", "rewards", "dones", "priorities")
# full boards without two equal neighbours: no move changes them and every action leaves the game over
DEAD = np.array([[1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1],
                 [3, 4, 3, 4, 4, 3, 4, 3, 3, 4, 3, 4, 4, 3, 4, 3],
                 [1, 2, 3, 4, 2, 3, 4, 5, 3, 4, 5, 6, 4, 5, 6, 7],
                 [7, 1, 7, 1, 1, 7, 1, 7, 7, 1, 7, 1, 1, 7, 1, 7]], dtype=np.uint8)
_NETS = {}


def g():
    import g2048
    return g2048


def net_of(dim_ff=32, layers=1, precision="f32"):
    key = (dim_ff, layers, precision)
    if key not in _NETS:
        torch.manual_seed(1000 + dim_ff + layers)
        model = RefSpelling(dim_ff, layers).eval()
        if layers > 1:
            distinct_layers(model.transformer.layers, 11)
        _NETS[key] = g().DeviceQNetwork(model.to(DEV), precision=precision)
    return _NETS[key]


def play(net, n, calls, fused, epsilon, capacity=256, cap=0, prepare=None, **beam):
    """A fresh buffer and collector, `prepare(collector, buffer)`, then one collect per entry of `calls`. Everything the calls
    leave behind, on the host."""
    buf = g().DeviceReplayBuffer(capacity, device=DEV, seed=3)
    col = g().DQNCollector(net, buf, n, seed=SEED, id_base=ID_BASE, max_episode_steps=cap, device=DEV)
    if prepare:
        prepare(col, buf)
    flags, indices = zip(*[col.collect(steps, epsilon, fused=fused, **beam) for steps in calls])
    torch.cuda.synchronize()
    out = {name: t.cpu() for name, t in zip(RING, buf._ring())}
    out.update(size=buf.size, head=buf.head, step_index=col.step_index, flags=torch.cat(flags).cpu(), indices=indices[-1].cpu(),
               boards=col.boards.cpu(), scores=col.scores.cpu(), moves=col.moves.cpu())
    return out, col, buf


def assert_same(fused, stepwise):
    assert fused.keys() == stepwise.keys()
    for k in fused:
        if isinstance(fused[k], int):
            assert fused[k] == stepwise[k], "%s: fused %d, stepwise %d" % (k, fused[k], stepwise[k])
        else:
            assert guard.same_bits(fused[k], stepwise[k]), "%s differs between the fused and the stepwise collector" % k


def both(net, n, calls, epsilon, **kw):
    """(the stepwise result, its collector, its buffer) after the fused result was found equal to it, bit for bit."""
    stepwise, col, buf = play(net, n, calls, False, epsilon, **kw)
    fused, _, _ = play(net, n, calls, True, epsilon, **kw)
    assert_same(fused, stepwise)
    return stepwise, col, buf


def explored_of(net, r, n, steps, epsilon, start=0):
    """(explored, exploit actions) (steps, n) of the transitions in slots start .. of an unwrapped ring, from the entry points."""
    from g2048 import ops
    states = r["states"][start:start + steps * n].to(DEV)
    exploit, q = net.act(states)
    exploit = exploit.clone()
    explored = torch.zeros(steps * n, dtype=torch.uint8, device=DEV)
    for t in range(steps):
        rows = slice(t * n, (t + 1) * n)
        ops.qnet_select_actions(q[rows], states[rows], epsilon, SEED, t, ID_BASE, explored=explored[rows])
    return explored.cpu().view(steps, n).bool(), exploit.cpu().view(steps, n)


def fresh_codes(step_index, ids, oracle):
    """The board an episode that ended at `step_index` goes on from: oracle.env_reset of the two EPISODE-domain draws."""
    k0, k1 = oracle.rng_keys(SEED, DOM_EPISODE, step_index)
    tiles = np.stack([oracle.env_reset(oracle.rng_draw(k0, k1, i, 0), oracle.rng_draw(k0, k1, i, 1)) for i in ids])
    return np.where(tiles > 0, np.log2(np.maximum(tiles, 1)), 0).astype(np.uint8)


def test_basics_against_the_stepwise_collector_and_the_oracle(oracle):
    n, steps, eps = 33, 6, 0.5
    dead = np.tile(DEAD, (2, 1))
    for a in range(4):           # on the CPU: every action leaves each of the eight boards finished
        _, _, _, fl = oracle.step_batch(dead, np.full(8, a, np.uint8), np.zeros(8, np.uint32), seed=SEED, step_index=0, id_base=ID_BASE)
        assert (fl & 1).all() and not (fl & 2).any()

    def prepare(col, buf):
        col.boards[:8] = torch.from_numpy(dead).to(DEV)

    r, _, _ = both(net_of(), n, [steps], eps, prepare=prepare)
    assert r["size"] == steps * n and r["head"] == 0 and r["step_index"] == steps
    flags = r["flags"].view(steps, n)
    assert int((flags[:-1] & 1).sum()) >= 8 and bool((flags[0, :8] & 1).all()), "the resets at t = 0 that are then played on"
    assert bool(((flags & 2) == 0).any()), "no invalid move"
    explored, exploit = explored_of(net_of(), r, n, steps, eps)
    actions = r["actions"][:steps * n].view(steps, n)
    assert bool(explored.any()) and bool((~explored).any()), "explored and exploited actions"
    assert torch.equal(actions[~explored], exploit[~explored])
    assert torch.equal(r["indices"], torch.arange(steps * n)) and bool((r["priorities"][:steps * n] == 1.0).all())
    assert bool((r["priorities"][steps * n:] == 0).all()) and bool((r["states"][steps * n:] == 0).all())
    # the stepwise yardstick itself against the CPU oracle: every transition, the resets and what is played on afterwards
    boards, scores = r["states"][:n].numpy().copy(), np.zeros(n, np.uint32)
    ids = range(ID_BASE, ID_BASE + n)
    for t in range(steps):
        rows = slice(t * n, (t + 1) * n)
        assert np.array_equal(r["states"][rows].numpy(), boards), t
        nxt, scores, reward, fl = oracle.step_batch(boards, actions[t].numpy(), scores, seed=SEED, step_index=t, id_base=ID_BASE)
        assert np.array_equal(r["next_states"][rows].numpy(), nxt) and np.array_equal(flags[t].numpy(), fl), t
        assert np.array_equal(r["rewards"][rows].numpy(), reward.astype(np.float32)) and np.array_equal(r["dones"][rows].numpy(), fl & 1), t
        done = (fl & 1).astype(bool)
        boards = np.where(done[:, None], fresh_codes(t, ids, oracle), nxt)
        scores = np.where(done, 0, scores).astype(np.uint32)
    assert np.array_equal(r["boards"].numpy(), boards) and np.array_equal(r["scores"].numpy().astype(np.uint32), scores)


def test_wrap_eviction_and_a_maximum_that_the_call_evicts():
    n, steps, capacity = 33, 3, 100
    seen = {}

    def prepare(col, buf):
        col.prefill(90)
        buf.update_priorities(torch.tensor([5, 89], device=DEV), torch.tensor([3.7, 0.25], device=DEV))
        seen["before"] = {name: t.cpu().clone() for name, t in zip(RING, buf._ring())}
        assert (buf.size, buf.head) == (90, 0)

    r, _, _ = both(net_of(), n, [steps], 0.5, capacity=capacity, prepare=prepare)
    before = seen["before"]
    m = before["priorities"].max()
    assert float(m) == float(before["priorities"][5]) and 3.69 < float(m) < 3.71, "the maximum sits on entry 5, which this call evicts"
    assert r["size"] == capacity and r["head"] == 89, "99 entries behind 90 in a ring of 100: 89 evicted"
    new = np.r_[90:100, 0:89]
    assert guard.same_bits(r["priorities"][new], m.expand(99)), "every new entry has the evicted maximum's bits"
    for name in RING:
        assert guard.same_bits(r[name][89], before[name][89]), "the one survivor's %s changed" % name
    assert float(r["priorities"][89]) < 1.0
    assert torch.equal(r["indices"], torch.arange(1, 100))
    # entry k = t n + i sits at slot (90 + k) % 100: the states of step 1 are what step 0 went on from, none of them finished
    assert torch.equal(r["states"][new][n:2 * n], r["next_states"][new][:n]) and not bool(r["dones"][new].any())


def test_the_episode_cap_restarts_every_second_move(oracle):
    n, eps = 33, 0.5
    r, col, _ = both(net_of(), n, [5], eps, cap=2)
    assert not bool(r["dones"].any()) and not bool((r["flags"] & 1).any()), "a truncated episode's done stays 0"
    ids = range(ID_BASE, ID_BASE + n)
    states, nxt = r["states"][:5 * n].view(5, n, 16), r["next_states"][:5 * n].view(5, n, 16)
    for t in (1, 3):            # the second move of an episode: the env goes on from the fresh board of (t, id)
        assert np.array_equal(states[t + 1].numpy(), fresh_codes(t, ids, oracle)), t
        assert not bool((states[t + 1] == nxt[t]).all(dim=1).any())
    for t in (0, 2):
        assert torch.equal(states[t + 1], nxt[t])
    assert torch.equal(r["boards"], nxt[4]) and bool((r["moves"] == 1).all())
    split_fused, _, _ = play(net_of(), n, [3, 2], True, eps, cap=2)
    split_stepwise, _, _ = play(net_of(), n, [3, 2], False, eps, cap=2)
    for split in (split_fused, split_stepwise):
        for k in r:
            if k not in ("flags", "indices"):
                assert r[k] == split[k] if isinstance(r[k], int) else guard.same_bits(r[k], split[k]), k
        assert torch.equal(split["flags"].view(-1), r["flags"].view(-1))


@pytest.mark.parametrize("n,shape,precision,eps", [(1, (32, 1), "f32", 0.5), (32, (32, 1), "f32", 0.5), (33, (64, 2), "bf16", 0.5),
                                                   (33, (32, 1), "f32", 0.0), (33, (32, 1), "f32", 1.0)],
                         ids=["one_env", "one_full_wavefront", "bf16_64x2", "epsilon_0", "epsilon_1"])
def test_shapes_precisions_and_the_ends_of_epsilon(n, shape, precision, eps):
    net, steps = net_of(*shape, precision), 4
    r, _, _ = both(net, n, [steps], eps)
    assert r["size"] == steps * n and tuple(r["flags"].shape) == (steps, n) and tuple(r["boards"].shape) == (n, 16)
    assert net.precision == precision and (net.dim_ff, net.n_layers) == shape
    explored, exploit = explored_of(net, r, n, steps, eps)
    actions = r["actions"][:steps * n].view(steps, n)
    if eps == 0.0:
        assert not bool(explored.any()) and torch.equal(actions, exploit)
    elif eps == 1.0:
        assert bool(explored.all()) and not torch.equal(actions, exploit)
    else:
        assert torch.equal(actions[~explored], exploit[~explored])
    if precision == "bf16":
        q32 = net_of(*shape, "f32")(r["states"][:n].to(DEV)).cpu()
        assert not torch.equal(net(r["states"][:n].to(DEV)).cpu(), q32), "the bf16 blob gave the f32 network's Q-values"


def test_beam_search_against_act_beam():
    from g2048 import ops
    n, steps, eps, beam = 33, 4, 0.3, dict(use_beam_search=True, beam_width=3, search_depth=2, threshold=4)
    crowded = random_boards(40, seed=2)[5:21]                  # 6 .. 14 tiles up to 2048: most of them are boards the search plans
    assert ((crowded > 0).sum(axis=1) >= 8).sum() >= 8

    def prepare(col, buf):
        col.boards[:16] = torch.from_numpy(crowded).to(DEV)

    net = net_of()
    r, _, _ = both(net, n, [steps], eps, prepare=prepare, **beam)
    states = r["states"][:steps * n].to(DEV)
    q = net(states).clone()
    planned_all, plain_all = [], []
    for t in range(steps):
        rows = slice(t * n, (t + 1) * n)
        acts, planned, _ = ops.qnet_beam_actions(q[rows], states[rows], None, 3, 2, 4, 0.99, eps, SEED, t, ID_BASE)
        plain, _ = ops.qnet_select_actions(q[rows], states[rows], eps, SEED, t, ID_BASE)
        assert torch.equal(acts.cpu(), r["actions"][rows]), t
        planned_all.append(planned.cpu())
        plain_all.append(plain.cpu())
    planned = torch.cat(planned_all).bool()
    assert bool(planned.any()) and bool((~planned).any()), "planned and unplanned boards"
    assert not torch.equal(torch.cat(plain_all), r["actions"][:steps * n]), "the search decided nothing the argmax would not have"


def test_guard_bands_round_everything_the_call_writes():
    from g2048 import ops
    n, steps, capacity = 33, 3, 100
    net = net_of()
    buf = g().DeviceReplayBuffer(capacity, device=DEV, seed=3)
    col = g().DQNCollector(net, buf, n, seed=SEED, id_base=ID_BASE, max_episode_steps=2, device=DEV)
    col.prefill(90)
    col.collect(1, 0.5)                     # 123 entries pushed: the ring has wrapped, head 23
    torch.cuda.synchronize()
    assert (buf.size, buf.head) == (100, 23)
    ring0 = [t.cpu() for t in buf._ring()]
    boards0, scores0, moves0 = col.boards.cpu(), col.scores.cpu(), col.moves.cpu()

    def call(S):
        ring = [S.inp(name, t, align=16 if t.dim() == 2 else t.element_size()) for name, t in zip(RING, ring0)]
        boards, scores, moves = S.inp("boards", boards0, align=16), S.inp("scores", scores0, align=4), S.inp("moves", moves0, align=4)
        packed = S.inp("packed", net.packed, align=16)
        flags = S.out("flags", steps, (n,), torch.uint8)
        workspace = S.out("workspace", ops.qnet_collect_workspace_bytes(n), (), torch.uint8, align=4)
        size, head, _ = ops.qnet_collect(boards, scores, moves, packed, net.dim_ff, net.n_layers, *ring, 100, 23, steps, epsilon=0.5,
                                         seed=SEED, step_index0=1, id_base=ID_BASE, max_episode_steps=2, flags=flags, workspace=workspace)
        assert (size, head) == (100, (23 + 99) % 100)
        return dict(zip(RING, ring), boards=boards, scores=scores, moves=moves, flags=flags)

    out = guard.twice(DEV, call)
    # 99 transitions into 100 slots: the newest entry before the call, at slot 22, is the one that is left
    for name, t in zip(RING, ring0):
        assert guard.same_bits(out[name][22], t[22]), name
    assert not guard.same_bits(out["states"], ring0[0]) and bool((out["moves"] <= 1).all())
    col.collect(steps, 0.5, fused=False)    # the same call through the class, stepwise
    torch.cuda.synchronize()
    for name, t in zip(RING, buf._ring()):
        assert guard.same_bits(out[name], t.cpu()), name
    assert guard.same_bits(out["boards"], col.boards.cpu()) and guard.same_bits(out["moves"], col.moves.cpu())


def test_the_host_class_feeds_sample_prefill_and_refuses_too_many_transitions(oracle):
    from g2048 import ops
    net, n = net_of(), 33
    u = torch.linspace(0.0, 1.0, 64, dtype=torch.float64, device=DEV) * 0.999
    batches = []
    for fused in (True, False):
        _, col, buf = play(net, n, [3, 2], fused, 0.5, prepare=lambda col, buf: col.prefill(40))
        assert len(buf) == 40 + 5 * n
        (states, actions, rewards, nxt, dones), indices, weights, shaped = buf.sample(64, beta=0.4, u=u)
        batches.append([t.cpu() for t in (states, actions, rewards, nxt, dones, indices, weights, shaped)])
    for a, b in zip(*batches):
        assert guard.same_bits(a, b)
    assert len(set(batches[0][5].tolist())) > 32, "the draws spread over the buffer"

    buf = g().DeviceReplayBuffer(256, device=DEV, seed=3)
    col = g().DQNCollector(net, buf, n, seed=SEED, id_base=ID_BASE, device=DEV)
    indices = col.prefill(64)
    torch.cuda.synchronize()
    assert len(buf) == 64 and col.step_index == 0 and torch.equal(indices.cpu(), torch.arange(64))
    fresh, _ = ops.reset(64, SEED, 1, ID_BASE, device=DEV)
    assert torch.equal(buf.states[:64], fresh) and bool(((buf.states[:64] > 0).sum(dim=1) == 2).all()), "fresh boards: two tiles"
    assert torch.equal(buf.actions[:64], ops.synth_actions(64, SEED, 0, ID_BASE, device=DEV))
    assert len(set(buf.actions[:64].tolist())) == 4
    nxt, _, reward, fl = oracle.step_batch(fresh.cpu().numpy(), buf.actions[:64].cpu().numpy(), np.zeros(64, np.uint32), seed=SEED,
                                           step_index=0, id_base=ID_BASE)
    assert np.array_equal(buf.next_states[:64].cpu().numpy(), nxt) and np.array_equal(buf.rewards[:64].cpu().numpy(), reward.astype(np.float32))
    assert bool((buf.priorities[:64] == 1.0).all()) and np.array_equal(buf.dones[:64].cpu().numpy(), fl & 1)
    with pytest.raises(ValueError, match="exceed the buffer's capacity"):
        col.collect(8, 0.5)                  # 8 x 33 = 264 > 256
    with pytest.raises(ValueError, match="exceed the buffer's capacity"):
        col.collect(8, 0.5, fused=False)
    with pytest.raises(ValueError, match="search_depth 1"):
        col.collect(1, 0.5, use_beam_search=True, search_depth=1)
    assert len(buf) == 64 and col.step_index == 0, "a refused call changed the collector"
