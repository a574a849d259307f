"""g2048_policy_forward on the MI355X: the trained reference checkpoint against the reference's own recorded outputs, random
weights against a NumPy f64 forward at ragged sizes, determinism, in-place refresh under a captured rollout graph, the
RolloutCollector boards hook, and argument validation."""

import numpy as np
import pytest
import torch

from test_policy_host import RefLayout, golden_modules, numpy_forward, perturb_bn, random_boards, state_dict_np

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = {"f32": dict(probs=2e-5, probs_mean=2e-5, values=1e-5), "bf16": dict(probs=1e-2, probs_mean=1e-3, values=3e-2)}


def check(precision, probs, values, want_p, want_v, what):
    probs = np.asarray(probs, np.float64)
    ep = np.abs(probs - want_p)
    t = TOL[precision]
    print("%s %s: probs max %.3g mean %.3g" % (what, precision, ep.max(), ep.mean()), end="")
    assert ep.max() <= t["probs"] and ep.mean() <= t["probs_mean"], what
    assert np.all(np.isfinite(probs)) and np.allclose(probs.sum(1), 1.0, atol=1e-5 if precision == "f32" else 1e-4)
    if values is not None:
        ev = np.abs(np.asarray(values, np.float64) - want_v).max() / np.abs(want_v).max()
        print("; values max %.3g of max|v| %.4g" % (ev, np.abs(want_v).max()), end="")
        assert ev <= t["values"], what
    print()


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_reference_checkpoint(precision):
    from g2048 import DevicePolicy
    g, actor, critic = golden_modules()
    pol = DevicePolicy(actor.to(DEV), critic.to(DEV), precision=precision)
    boards = torch.from_numpy(g["boards"]).to(DEV)
    p, v = pol(boards)
    check(precision, p.cpu().numpy(), v.cpu().numpy(), g["probs_batched"], g["values_batched"], "batched")
    k = g["probs_single"].shape[0]
    ps, vs = [], []
    for i in range(k):                           # batches of one row: the reference skips BatchNorm
        a, b = pol(boards[i:i + 1])
        ps.append(a.clone())
        vs.append(b.clone())
    check(precision, torch.cat(ps).cpu().numpy(), torch.cat(vs).cpu().numpy(), g["probs_single"], g["values_single"], "n=1")


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_random_weights_ragged_sizes_and_canaries(precision):
    from g2048 import DevicePolicy, ops
    gen = torch.Generator().manual_seed(2)
    torch.manual_seed(2)
    actor, critic = perturb_bn(RefLayout(4), gen), perturb_bn(RefLayout(1), gen)
    sda, sdc = state_dict_np(actor), state_dict_np(critic)
    pol = DevicePolicy(actor.to(DEV), critic.to(DEV), precision=precision)
    all_boards = random_boards(65537, 9)
    for n in (2, 63, 64, 65, 4096, 65537):
        b = torch.from_numpy(all_boards[:n]).to(DEV)
        x = all_boards[:n].astype(np.float32) / np.float32(15)
        probs = torch.full((n + 67, 4), 7.0, device=DEV)
        value = torch.full((n + 67, 1), 7.0, device=DEV)
        ops.policy_forward(b, pol.actor.blob(n), pol.critic.blob(n), precision, probs=probs[:n], value=value[:n])
        torch.cuda.synchronize()
        assert torch.all(probs[n:] == 7.0) and torch.all(value[n:] == 7.0), "rows past n were written (n = %d)" % n
        check(precision, probs[:n].cpu().numpy(), value[:n].cpu().numpy(), numpy_forward(sda, x, True, True),
              numpy_forward(sdc, x, True, False), "random n=%d" % n)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_two_launches_are_bit_identical(precision):
    from g2048 import DevicePolicy
    torch.manual_seed(4)
    gen = torch.Generator().manual_seed(4)
    pol = DevicePolicy(perturb_bn(RefLayout(4), gen).to(DEV), perturb_bn(RefLayout(1), gen).to(DEV), precision=precision)
    b = torch.from_numpy(random_boards(100003, 1)).to(DEV)
    p1, v1 = [t.clone() for t in pol(b)]
    p2, v2 = pol(b)
    assert torch.equal(p1, p2) and torch.equal(v1, v2)


def _collector_state(rc):
    return dict(boards=rc.env.boards.clone(), scores=rc.env.scores.clone(), t=rc.env.t)


def _start_from(rc, state):
    rc.env.boards.copy_(state["boards"])
    rc.env.scores.copy_(state["scores"])
    rc.env.t = state["t"]


def _traj(out):
    return {k: out[k].clone() for k in ("obs", "actions", "log_prob", "values", "rewards", "dones", "valid_mask", "last_obs")}


def test_graph_replay_after_refresh_uses_the_new_weights():
    from g2048 import DevicePolicy, RolloutCollector
    torch.manual_seed(6)
    gen = torch.Generator().manual_seed(6)
    actor, critic = perturb_bn(RefLayout(4), gen).to(DEV), perturb_bn(RefLayout(1), gen).to(DEV)
    pol = DevicePolicy(actor, critic)
    pol_old = DevicePolicy(actor, critic)        # keeps the weights before the optimizer step (never refreshed)
    n, T, seed = 4096, 16, 77
    rc = RolloutCollector(n, T, pol, device=DEV, seed=seed, use_graph=True)
    rc.collect()
    assert rc._graph is not None, "the collector did not capture its loop"
    state = _collector_state(rc)
    # one optimizer step on the modules, back to eval, re-pack in place
    opt = torch.optim.SGD(list(actor.parameters()) + list(critic.parameters()), lr=0.05)
    actor.train()
    critic.train()
    x = torch.rand(256, 16, device=DEV)
    loss = -(actor(x)[:, 0].log().mean()) + critic(x).pow(2).mean()
    opt.zero_grad()
    loss.backward()
    opt.step()
    actor.eval()
    critic.eval()
    pol.refresh()
    replayed = _traj(rc.collect())
    fresh = RolloutCollector(n, T, pol, device=DEV, seed=seed, use_graph=True)
    _start_from(fresh, state)
    want = _traj(fresh.collect())
    assert fresh._graph is not None
    for k in want:
        assert torch.equal(replayed[k], want[k]), "replay after refresh differs from a fresh capture in %s" % k
    old = RolloutCollector(n, T, pol_old, device=DEV, seed=seed, use_graph=True)
    _start_from(old, state)
    before = _traj(old.collect())
    assert torch.equal(before["obs"][0], replayed["obs"][0])           # same starting state ...
    assert not torch.equal(before["log_prob"], replayed["log_prob"])   # ... but the replay ran the new weights
    assert not torch.equal(before["values"], replayed["values"])


def test_rollout_boards_hook_matches_an_observation_wrapper():
    from g2048 import DevicePolicy, RolloutCollector
    torch.manual_seed(8)
    gen = torch.Generator().manual_seed(8)
    pol = DevicePolicy(perturb_bn(RefLayout(4), gen).to(DEV), perturb_bn(RefLayout(1), gen).to(DEV))

    class ObsWrapper(torch.nn.Module):           # a plain torch policy: re-packs the float observation, calls the same kernel
        def forward(self, obs):
            return pol(torch.round(obs * 15).to(torch.uint8).contiguous())

    n, T = 8192, 12
    for use_graph in (False, True):
        a = _traj(RolloutCollector(n, T, pol, device=DEV, seed=5, use_graph=use_graph).collect())
        b = _traj(RolloutCollector(n, T, ObsWrapper(), device=DEV, seed=5, use_graph=use_graph).collect())
        for k in a:
            assert torch.equal(a[k], b[k]), "%s differs (use_graph=%s)" % (k, use_graph)
        assert a["values"].abs().sum() > 0


def test_bad_arguments_launch_nothing():
    from g2048 import DevicePolicy, _lib, ops
    L = _lib.lib()
    torch.manual_seed(1)
    pol = DevicePolicy(RefLayout(4).eval().to(DEV), RefLayout(1).eval().to(DEV))
    b = torch.from_numpy(random_boards(64, 2)).to(DEV)
    probs = torch.full((64, 4), 3.0, device=DEV)
    value = torch.full((64, 1), 3.0, device=DEV)
    a, c = pol.actor.blob(64), pol.critic.blob(64)
    cases = [
        ((b.data_ptr(), a.data_ptr(), c.data_ptr(), probs.data_ptr(), value.data_ptr(), 64, 5, None), b"opts"),
        ((b.data_ptr() + 4, a.data_ptr(), c.data_ptr(), probs.data_ptr(), value.data_ptr(), 64, 0, None), b"misaligned"),
        ((b.data_ptr(), a.data_ptr() + 8, None, probs.data_ptr(), None, 64, 0, None), b"misaligned"),
        ((b.data_ptr(), a.data_ptr(), c.data_ptr(), probs.data_ptr(), None, 64, 0, None), b"both"),
        ((b.data_ptr(), None, None, probs.data_ptr(), None, 64, 0, None), b"null pointer"),
    ]
    for args, msg in cases:
        assert L.g2048_policy_forward(*args) == -1
        assert msg in L.g2048_last_error()
    packed = torch.full((ops.policy_packed_bytes("f32", 4),), 9, dtype=torch.uint8, device=DEV)
    plain = torch.zeros(45504 + 65 * 4, device=DEV)
    assert L.g2048_policy_pack(plain.data_ptr(), 4, 3, packed.data_ptr(), None) == -1 and b"precision" in L.g2048_last_error()
    assert L.g2048_policy_pack(plain.data_ptr(), 2, 0, packed.data_ptr(), None) == -1 and b"n_out" in L.g2048_last_error()
    torch.cuda.synchronize()
    assert torch.all(probs == 3.0) and torch.all(value == 3.0) and torch.all(packed == 9), "a refused call wrote output"
    with pytest.raises(TypeError):
        pol(b.to(torch.int32))
    with pytest.raises(ValueError):
        ops.policy_forward(b, a, c, "f32", probs=probs[:10])
