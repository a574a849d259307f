"""DQNAgent.train_step as examples/dqn_replay.py --train strings it together, four rounds in a closed loop on the MI355X:
buf.sample -> buf.boards -> g2048.dqn_targets -> online.loss_and_grad -> clip_grad_norm_ -> AdamW.step -> CosineAnnealingLR.step ->
buf.update_priorities -> online.refresh, the target network synchronised after the second round. Small throughout: dim_ff 160 (one
main group and one tail step of the products), 2 layers, a batch of 33 out of 90 transitions in a ring of 100, early boards (codes
0..3), online and target two different random-init modules.

Every round is checked against CPU copies deep-copied from the device modules at the round's start, so rounds 1 - 3 pass only if
refresh() delivered every tensor to the batch path and the buffers the networks reuse per (n, stream) carry nothing over:
* targets and next actions against forward_batch_reference of the float64 copies, by the convention of
  test_dqn_targets_against_the_reference, no row left out (every row is clear of a tie with these seeds);
* loss, td and every gradient against the stock module's float64 autograd on the device's own float32 targets and weights, within
  8 x the float32 copy's error of that round (the convention of test_gpu_qnet_grad.py);
* clipping at half of round 0's float64 gradient norm: the returned norm, the norm afterwards, the eps slots;
* the optimiser step against a float64 CPU AdamW + scheduler fed the device's pre-step weights and clipped gradients, within 8 x
  the deviation of a float32 CPU mirror fed the same way; net.plain bit for bit the module after refresh();
* the priorities written back (float32 td + 1e-5, the latest duplicate wins, everything else untouched);
* the target network: different before the sync, bit-equal right after it, different again after the next online step.

Measured on an MI355X: see the head of test_closed_loop_of_four_rounds."""
import copy

import numpy as np
import pytest
import torch

import per_ref
import qnet_grad_ref as R
from test_gpu_qnet_batch import F32_FACTOR, device_net
from test_gpu_qnet_grad import DEV, check, split, to_dev
from test_policy_host import random_boards
from test_qnet_host import random_model, tiles

pytestmark = pytest.mark.gpu

DIM_FF, LAYERS, BATCH, CAPACITY, PUSHED, ROUNDS, GAMMA = 160, 2, 33, 100, 90, 4, 0.99
ONLINE_SEED, TARGET_SEED, DATA_SEED = 2, 3, 23
SYNC_AFTER = 1                                             # the target is synchronised at the end of this round


def transitions(seed=DATA_SEED):
    """(states, actions, rewards float32, next_states, dones) of the 90 pushed transitions: early boards, every action, about one
    done flag in ten. The rewards cancel most of train_step's shaping bonus (8 .. 18 on such boards, shaped = 0.1 reward + bonus), so
    that the shaped rewards scatter around 0 like the Q of a random-init module and both Huber branches are taken."""
    rng = np.random.default_rng(seed)
    states, nxt = (random_boards(PUSHED, seed) % 4).astype(np.uint8), (random_boards(PUSHED, seed + 1) % 4).astype(np.uint8)
    actions = rng.permutation(np.arange(PUSHED) % 4).astype(np.uint8)
    bonus = per_ref.shaped_rewards(states, nxt, np.zeros(PUSHED, np.float32)).astype(np.float64)
    rewards = (10.0 * (rng.normal(0.0, 1.2, PUSHED) - bonus)).astype(np.float32)
    dones = (rng.random(PUSHED) < 0.1).astype(np.uint8)
    assert set(actions) == {0, 1, 2, 3} and 4 <= dones.sum() <= 14
    return states, actions, rewards, nxt, dones


def draws(seed=DATA_SEED):
    """The rounds' explicit uniforms for buf.sample."""
    return np.random.default_rng(seed + 100).random((ROUNDS, BATCH))


def beta_of(round_index):
    return 0.4 + 0.6 * min(round_index / 1000.0, 1.0)


def cpu_copies(net):
    m = copy.deepcopy(net.model).cpu()
    return copy.deepcopy(m).double(), m.float()


def q_pair(m64, m32, codes):
    """(float64 batch forward by forward_batch_reference, the stock module's float32 batch call) on uint8 codes."""
    from g2048 import qnet
    with torch.no_grad():
        f32 = m32(tiles(codes, torch.float32)).numpy().astype(np.float64)
    return qnet.forward_batch_reference(qnet.parse(m64), torch.from_numpy(codes)).numpy(), f32


def check_targets(what, targets, actions, shaped, dones, on, tg, next_codes):
    """The convention of test_dqn_targets_against_the_reference on the round's own copies, with no row left out."""
    q, q32 = q_pair(*on, next_codes)
    qt, qt32 = q_pair(*tg, next_codes)
    bound, t_bound = F32_FACTOR * np.abs(q32 - q).max(), F32_FACTOR * np.abs(qt32 - qt).max()
    srt = np.sort(q, axis=1)
    gap = srt[:, 3] - srt[:, 2]
    assert np.all(gap > 2 * bound), "%s: a row within twice the Q bound of a tie (gap %.3g, bound %.3g): take another seed" % (what, gap.min(), bound)
    want_actions = q.argmax(1)
    want = shaped.astype(np.float64) + (1.0 - dones) * GAMMA * qt[np.arange(len(q)), want_actions]
    err = np.abs(targets.astype(np.float64) - want)
    allowed = GAMMA * t_bound + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    print("%s: targets: smallest gap between the top two Q %.3g (twice the bound: %.3g), target error %.3g (allowed %.3g)"
          % (what, gap.min(), 2 * bound, err.max(), allowed.min()))
    assert np.array_equal(actions, want_actions), what
    assert np.all(err <= allowed), what
    assert np.array_equal(targets[dones == 1], shaped[dones == 1]), what


def set_mirror(model, optimizer, weights, grads):
    """One isolated step of a CPU mirror: its parameters := the device's pre-step weights, its gradients := the device's clipped
    gradients (its moment estimates are its own, so they follow the device's gradients round by round)."""
    with torch.no_grad():
        for p, w, g in zip(model.parameters(), weights, grads):
            p.copy_(torch.from_numpy(w).reshape(p.shape).to(p.dtype))
            p.grad = torch.from_numpy(g).reshape(p.shape).to(p.dtype)
    optimizer.step()
    return [p.detach().numpy().astype(np.float64).reshape(-1) for p in model.parameters()]


def ring_copy(buf):
    return [x.clone() for x in (buf.states, buf.next_states, buf.actions, buf.rewards, buf.dones)]


def test_closed_loop_of_four_rounds():
    """Measured on an MI355X (rounds 0 - 3): gradients 0.61, 0.82, 0.69, 0.80 x the float32 copy's error (every tensor at most
    1.57 x its own), the optimiser step 1.00 x the float32 mirror's deviation in every round (7.8e-8 of max|w|; bound 8 x both);
    clipping acted in rounds 0 and 1 and not in 2 and 3; the smallest gap between the top two Q was 0.037 against twice the bound
    7.7e-6."""
    import g2048
    online, target = device_net(random_model(ONLINE_SEED, DIM_FF, LAYERS)), device_net(random_model(TARGET_SEED, DIM_FF, LAYERS))
    assert (online.dim_ff, online.n_layers) == (DIM_FF, LAYERS)
    buf = g2048.DeviceReplayBuffer(CAPACITY, alpha=0.6, device=DEV, seed=1)
    states, actions, rewards, nxt, dones = transitions()
    buf.push(*to_dev(states, actions, rewards, nxt, dones))
    assert len(buf) == PUSHED
    assert online.attach_grads() is online.grad
    params = list(online.model.parameters())
    optimizer = torch.optim.AdamW(params, lr=1e-3, weight_decay=1e-4)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=10000, eta_min=1e-5)
    mirrors = []
    for dtype in (torch.float64, torch.float32):
        m = copy.deepcopy(online.model).cpu().to(dtype)
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-4)
        mirrors.append((m, opt, torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=10000, eta_min=1e-5)))
    slices, eps_at, _ = R.plain_slices(online.parsed)
    eps_plain = online.plain[eps_at].clone()
    assert len(eps_at) == 2 * LAYERS and torch.all(eps_plain > 0)
    max_norm, probe, duplicates = None, None, 0

    for rnd, u in enumerate(draws()):
        what = "round %d" % rnd
        on, tg = cpu_copies(online), cpu_copies(target)
        (_, acts, _, _, done_f), indices, weights, shaped = buf.sample(BATCH, beta=beta_of(rnd), u=to_dev(u)[0])
        boards, next_boards = buf.boards(indices)
        idx = indices.cpu().numpy()
        assert np.array_equal(boards.cpu().numpy(), states[idx]) and np.array_equal(next_boards.cpu().numpy(), nxt[idx]), what
        assert np.array_equal(acts.cpu().numpy(), actions[idx].astype(np.int64)) and np.array_equal(done_f.cpu().numpy(), dones[idx].astype(np.float32))
        duplicates += BATCH - len(np.unique(idx))
        if probe is None:
            probe = boards.clone()

        # ---- targets and next actions
        targets, next_actions = g2048.dqn_targets(online, target, next_boards, shaped, done_f, GAMMA)
        t_np, w_np = targets.cpu().numpy(), weights.cpu().numpy()
        check_targets(what, t_np, next_actions.cpu().numpy(), shaped.cpu().numpy(), done_f.cpu().numpy(), on, tg, nxt[idx])

        # ---- loss, td, gradients: the stock module's autograd on the device's own float32 targets and weights
        loss, td, q = online.loss_and_grad(boards, acts, targets, weights)
        a_np = acts.cpu().numpy()
        want, f32 = (R.stock_loss_grad(m, states[idx], a_np, t_np, w_np) for m in on)
        grads, eps = split(online, online.grad)
        assert np.all(eps == 0), what
        td_np = td.cpu().numpy()
        check((float(loss), td_np.astype(np.float64), None, grads), want, f32, True, what)
        assert torch.equal(q, online.forward_batch(boards)), what
        assert all(torch.equal(p.grad.reshape(-1), online.grad[o:o + k]) for p, (o, k) in zip(params, slices)), "a .grad is no longer a view"

        # ---- clipping
        if max_norm is None:
            max_norm = 0.5 * float(np.sqrt(sum(np.sum(g * g) for g in want[3])))
        before = float(online.grad.norm())
        norm = float(torch.nn.utils.clip_grad_norm_(params, max_norm=max_norm))
        after = float(online.grad.norm())
        print("%s: gradient norm %.4g, max_norm %.4g: clipping %s" % (what, norm, max_norm, "acted" if norm > max_norm else "did not act"))
        assert abs(norm - before) <= 1e-6 * before, (what, norm, before)
        assert abs(after - min(norm, max_norm)) <= 1e-5 * min(norm, max_norm), (what, after, norm, max_norm)
        assert rnd > 0 or norm > max_norm, "clipping must act in round 0"
        clipped, eps = split(online, online.grad)
        assert np.all(eps == 0), "%s: clipping moved a LayerNorm-eps slot of grad" % what

        # ---- the optimiser step against the CPU mirrors
        pre = [p.detach().numpy().astype(np.float64).reshape(-1) for p in on[1].parameters()]
        optimizer.step()                                   # no zero_grad: the next loss_and_grad overwrites
        scheduler.step()
        post = [p.detach().cpu().numpy().astype(np.float64).reshape(-1) for p in params]
        s64, s32 = (set_mirror(m, opt, pre, clipped) for m, opt, _ in mirrors)
        for _, _, sched in mirrors:
            sched.step()
        assert optimizer.param_groups[0]["lr"] == pytest.approx(mirrors[0][1].param_groups[0]["lr"], rel=1e-12)
        top = max(np.abs(x).max() for x in s64)
        e_dev, e_f32 = (max(np.abs(x - y).max() for x, y in zip(s, s64)) / top for s in (post, s32))
        moved = max(np.abs(x - y).max() for x, y in zip(post, pre))
        print("%s: optimiser step: weights moved by up to %.3g; device %.3g of max|w| from the float64 mirror = %.2f x the float32 "
              "mirror's %.3g (bound %.0f x)" % (what, moved, e_dev, e_dev / e_f32, e_f32, F32_FACTOR))
        assert 0.5e-3 < moved < 1.5e-3, what
        assert e_f32 > 0 and e_dev <= F32_FACTOR * e_f32, what

        # ---- priorities
        prio, ring = buf.logical_priorities().cpu().numpy(), ring_copy(buf)
        buf.update_priorities(indices, td)
        want_prio = prio.copy()
        for i, v in zip(idx, td_np.astype(np.float32) + np.float32(1e-5)):     # in order: the latest duplicate wins
            want_prio[i] = v
        assert np.array_equal(buf.logical_priorities().cpu().numpy(), want_prio), what
        assert not np.array_equal(want_prio[idx], prio[idx]) and all(torch.equal(x, y) for x, y in zip(ring, ring_copy(buf))), what

        # ---- refresh: the plain buffer is the module, bit for bit
        stale = online.plain.clone()
        online.refresh()
        flat = online.plain.clone()
        for p, (o, k) in zip(params, slices):
            flat[o:o + k] = p.detach().reshape(-1)
        assert torch.equal(online.plain, flat) and not torch.equal(online.plain, stale), what
        assert torch.equal(online.plain[eps_at], eps_plain), "%s: a LayerNorm-eps slot of plain changed" % what

        # ---- the target network
        if rnd == SYNC_AFTER:
            assert not torch.equal(target.forward_batch(probe), online.forward_batch(probe)), "the target equals the online network before the sync"
            target.model.load_state_dict(online.model.state_dict())
            target.refresh()
            assert torch.equal(target.plain, online.plain)
            assert torch.equal(target.forward_batch(probe), online.forward_batch(probe)), "a synchronised target is not bit-equal to the online network"
        if rnd == SYNC_AFTER + 1:
            assert not torch.equal(target.forward_batch(probe), online.forward_batch(probe)), "the target followed the online network's step"
    assert duplicates > 0, "no sampled index was duplicated in any round: the latest-wins rule was not run"
