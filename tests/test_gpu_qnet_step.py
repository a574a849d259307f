"""g2048_qnet_adamw_step on the MI355X: gradient clipping and AdamW over the Q-network's plain buffer in two launches, and the
three methods of DeviceQNetwork around it (attach_params, adamw_step, sync_from).

The kernel is checked against the yardstick qnet.adamw_step_reference (itself clip_grad_norm_ + torch.optim.AdamW to 1e-12:
tests/test_qnet_step_host.py) on the three smallest networks that give a 2-float tail ((32, 1) and (96, 3): an odd layer count), a
LayerNorm-eps pair in either half of a 16-byte group ((160, 2) and (96, 3): layers 0 and 1) and a total that is a multiple of 4
((160, 2)). Tolerance, the convention of test_gpu_qnet_train_round.py: per buffer max|device - y64| / max|y64| <= 8 x the same
measure of the float32 yardstick, both yardsticks fed the device's own pre-step state; the float32 deviation must be > 0. The norm is
held to 1e-6 of the float64 norm of the device's gradient, the clipped gradient to 4 float32 ulps an element of grad . c with c
formed in float64 from the device's own norm.

Measured on an MI355X: see the docstrings of the tests."""
import copy
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import qnet_grad_ref as R
from conftest import REPO
from test_gpu_qnet_batch import F32_FACTOR, check as check_q, device_net
from test_gpu_qnet_grad import DEV, check, split, to_dev
from test_gpu_qnet_train_round import (BATCH, CAPACITY, DIM_FF, GAMMA, LAYERS, ONLINE_SEED, TARGET_SEED, beta_of, check_targets,
                                       cpu_copies, draws, transitions)
from test_policy_host import random_boards
from test_qnet_host import random_model

pytestmark = pytest.mark.gpu

SHAPES = [(32, 1), (160, 2), (96, 3)]
IDS = ["ff%d-L%d" % s for s in SHAPES]
MAX_NORM, LR, WEIGHT_DECAY, CANARY = 10.0, 1e-3, 1e-4, 64
NORM_FACTORS = (2.0, 1.0, 0.5)                              # the gradient norm as a multiple of MAX_NORM, step by step
EPS_BASE = 139616


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def test_the_shapes_cover_the_tail_both_halves_of_a_group_and_a_whole_total():
    """No device work: what the issue chose the three shapes for."""
    from g2048 import ops
    totals = {s: ops.qnet_plain_floats(*s) for s in SHAPES}
    assert totals[(32, 1)] % 4 == 2 and totals[(96, 3)] % 4 == 2 and totals[(160, 2)] % 4 == 0
    for ff, layers in SHAPES:
        block = 66690 + 257 * ff
        assert block % 4 == 2 and EPS_BASE % 4 == 0
    halves = {(EPS_BASE + (l + 1) * (66690 + 257 * ff) - 2) % 4 for ff, layers in SHAPES[1:] for l in range(layers)}
    assert halves == {0, 2}


@functools.lru_cache(maxsize=None)
def shape_case(dim_ff, layers):
    """(plain float32, [gradient float32 per step], eps offsets) of a shape: random_model's weights in the plain layout, seeded
    random gradients with the LayerNorm-eps slots 0 and the norm NORM_FACTORS x MAX_NORM (shared, never modified)."""
    from g2048 import qnet
    parsed = qnet.parse(random_model(2, dim_ff, layers))
    _, eps_at, total = R.plain_slices(parsed)
    plain = qnet.flatten(parsed).clone()
    rng = np.random.default_rng(100 + dim_ff)
    grads = []
    for factor in NORM_FACTORS:
        g = rng.normal(0.0, 1.0, total) * np.exp(rng.normal(0.0, 2.0, total))          # magnitudes over several decades
        g[eps_at] = 0.0
        grads.append(torch.from_numpy((g * (factor * MAX_NORM / np.linalg.norm(g))).astype(np.float32)))
    assert total % 4 in (0, 2) and plain.numel() == total
    return plain, grads, eps_at


class Canaried:
    """Four buffers, the norm and the workspace as slices of larger device tensors filled with 7.0 (0x7 bytes): 64 floats before
    and after each buffer, the offsets multiples of 4 floats."""

    def __init__(self, total, workspace_bytes):
        self.total = total
        self.whole = [torch.full((total + 2 * CANARY,), 7.0, device=DEV) for _ in range(4)]
        self.buffers = [w[CANARY:CANARY + total] for w in self.whole]
        self.norm_whole = torch.full((3,), 7.0, device=DEV)
        self.norm = self.norm_whole[1]
        self.nb = workspace_bytes
        self.workspace = torch.full((workspace_bytes + 4096,), 7, dtype=torch.uint8, device=DEV)
        assert all(b.data_ptr() % 16 == 0 for b in self.buffers) and self.norm.dim() == 0

    def check(self, what):
        for w in self.whole:
            assert torch.all(bits(w[:CANARY]) == bits(torch.tensor([7.0]))) and torch.all(bits(w[CANARY + self.total:]) == bits(torch.tensor([7.0]))), \
                "%s: a canary next to a buffer was overwritten" % what
        assert self.norm_whole[0] == 7.0 and self.norm_whole[2] == 7.0, "%s: a canary next to the norm was overwritten" % what
        assert torch.all(self.workspace[self.nb:] == 7), "%s: the workspace was written past its stated size" % what


def yardsticks(pre, eps_at, step, max_norm):
    from g2048 import qnet
    return tuple(tuple(t.numpy().astype(np.float64) for t in qnet.adamw_step_reference(*pre, eps_at, LR, step, weight_decay=WEIGHT_DECAY,
                                                                                       max_norm=max_norm, dtype=dtype))
                 for dtype in (torch.float64, torch.float32))


def run_steps(dim_ff, layers, verify):
    """Three consecutive updates through ops.qnet_adamw_step on canaried slices; returns the bits of the four buffers at the end
    and of every step's norm."""
    from g2048 import ops
    plain0, grads, eps_at = shape_case(dim_ff, layers)
    total = plain0.numel()
    c = Canaried(total, ops.qnet_step_workspace_bytes(dim_ff, layers))
    plain, grad, m, v = c.buffers
    plain.copy_(plain0)
    m.zero_()
    v.zero_()
    norms, ratios = [], []
    for step, (g, factor) in enumerate(zip(grads, NORM_FACTORS), 1):
        what = "ff%d-L%d step %d" % (dim_ff, layers, step)
        grad.copy_(g)
        pre = [t.cpu() for t in c.buffers]
        out = ops.qnet_adamw_step(plain, grad, m, v, dim_ff, layers, LR, step, weight_decay=WEIGHT_DECAY, max_norm=MAX_NORM, norm=c.norm,
                                  workspace=c.workspace)
        assert out is c.norm
        norms.append(bits(c.norm).clone())
        if not verify:
            continue
        c.check(what)
        post = [t.cpu() for t in c.buffers]
        norm = float(c.norm)
        norm64 = float(np.linalg.norm(pre[1].numpy().astype(np.float64)))
        assert abs(norm - norm64) <= 1e-6 * norm64 and norm64 == pytest.approx(factor * MAX_NORM, rel=1e-6), (what, norm, norm64)
        y64, y32 = yardsticks(pre, eps_at, step, MAX_NORM)
        row = []
        for name, i in (("plain", 0), ("exp_avg", 2), ("exp_avg_sq", 3)):
            top = np.abs(y64[i]).max()
            e_dev, e_f32 = np.abs(post[i].numpy().astype(np.float64) - y64[i]).max() / top, np.abs(y32[i] - y64[i]).max() / top
            row.append(e_dev / e_f32 if e_f32 > 0 else np.inf)
            print("%s: %s %.3g of the largest entry from the float64 yardstick = %.2f x the float32 yardstick's %.3g (bound %.0f x)"
                  % (what, name, e_dev, row[-1], e_f32, F32_FACTOR))
            assert e_f32 > 0 and e_dev <= F32_FACTOR * e_f32, (what, name)
        ratios.append(row)
        # the gradient left behind: grad . c, c in float64 from the device's own norm
        coef = min(1.0, MAX_NORM / (np.float64(np.float32(norm)) + 1e-6))
        g_pre, g_post = pre[1].numpy(), post[1].numpy()
        assert (coef < 1.0) == (factor >= 1.0), (what, coef)
        if coef == 1.0:
            assert np.array_equal(g_post.view(np.int32), g_pre.view(np.int32)), "%s: an unclipped gradient changed" % what
        else:
            want = g_pre.astype(np.float64) * coef
            ulps = np.abs(g_post.astype(np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            print("%s: clipped gradient within %.2f float32 ulps of grad . c (c = %.9g)" % (what, ulps.max(), coef))
            assert ulps.max() <= 4.0, what
        assert np.array_equal(post[0].numpy()[eps_at].view(np.int32), pre[0].numpy()[eps_at].view(np.int32)), "%s: an eps slot of plain changed" % what
        assert all(pre[0].numpy()[eps_at] > 0)
        for i in (1, 2, 3):
            assert not post[i].numpy()[eps_at].any(), "%s: an eps slot of buffer %d is not 0" % (what, i)
        moved = np.abs(post[0].numpy().astype(np.float64) - pre[0].numpy()).max()
        assert 0.5 * LR < moved < 1.5 * LR, (what, moved)
    return [bits(t).clone() for t in c.buffers], norms, ratios


@pytest.mark.parametrize("dim_ff, layers", SHAPES, ids=IDS)
def test_three_steps_against_the_yardstick_with_canaries_and_bit_for_bit_twice(dim_ff, layers):
    """Measured on an MI355X, all three shapes and all three steps: weights, exp_avg and exp_avg_sq each 1.00 x the float32
    yardstick's deviation from the float64 one (weights 7.7e-8 .. 7.8e-8 of max|w|, exp_avg 1.6e-8 .. 9.4e-8, exp_avg_sq 1.4e-8 ..
    1.3e-7; bound 8 x); the clipped gradient within 0.58 float32 ulps of grad . c at c = 0.49999998 (step 1) and 0.68 at c =
    0.9999999 (step 2), bit-equal at c = 1 (step 3); the second run bit-equal in all four buffers and the norms."""
    first, norms, ratios = run_steps(dim_ff, layers, verify=True)
    again, norms_again, _ = run_steps(dim_ff, layers, verify=False)
    assert all(torch.equal(a, b) for a, b in zip(first, again)), "two runs from the same state differ in a buffer"
    assert all(torch.equal(a, b) for a, b in zip(norms, norms_again)), "two runs from the same state differ in a norm"
    print("ff%d-L%d: worst multiple of the float32 yardstick's deviation %.2f" % (dim_ff, layers, max(max(r) for r in ratios)))


@pytest.mark.parametrize("value, where", [(float("inf"), 5), (float("-inf"), -1), (float("nan"), 70001), (float("nan"), -1)],
                         ids=["inf-head", "-inf-tail", "nan-middle", "nan-tail"])
def test_a_gradient_that_is_not_finite_changes_nothing(value, where):
    """(32, 1): the bad element in the first group, in the middle and in the 2-float tail. All four buffers keep their bits."""
    from g2048 import ops
    dim_ff, layers = SHAPES[0]
    plain0, grads, _ = shape_case(dim_ff, layers)
    c = Canaried(plain0.numel(), ops.qnet_step_workspace_bytes(dim_ff, layers))
    plain, grad, m, v = c.buffers
    plain.copy_(plain0)
    grad.copy_(grads[0])
    m.copy_(grads[1] * 0.1)
    v.copy_(grads[2] * grads[2])
    grad[where] = value
    pre = [bits(t).clone() for t in c.buffers]
    norm = ops.qnet_adamw_step(plain, grad, m, v, dim_ff, layers, LR, 3, weight_decay=WEIGHT_DECAY, max_norm=MAX_NORM, norm=c.norm,
                               workspace=c.workspace)
    assert not np.isfinite(float(norm))
    assert all(torch.equal(a, bits(b)) for a, b in zip(pre, c.buffers)), "a buffer changed although the norm is not finite"
    c.check("not finite")


def test_max_norm_none_leaves_the_gradient_alone():
    from g2048 import ops
    dim_ff, layers = SHAPES[1]
    plain0, grads, _ = shape_case(dim_ff, layers)
    plain, grad = to_dev(plain0.numpy(), (grads[0] * 3).numpy())
    m, v = torch.zeros_like(plain), torch.zeros_like(plain)
    before = bits(grad).clone()
    norm = ops.qnet_adamw_step(plain, grad, m, v, dim_ff, layers, LR, 1, max_norm=None)
    norm64 = float(np.linalg.norm(grad.cpu().numpy().astype(np.float64)))
    assert norm64 > 5 * MAX_NORM and abs(float(norm) - norm64) <= 1e-6 * norm64
    assert torch.equal(bits(grad), before), "max_norm=None clipped"
    assert not torch.equal(plain.cpu(), plain0) and m.any() and v.any()


def early_inputs(model, n=33, seed=11):
    boards = (random_boards(n, seed) % 4).astype(np.uint8)
    a, t, w = R.case_inputs(copy.deepcopy(model).cpu().double(), boards)
    return to_dev(boards, a, t, w)


def module_is_plain(net):
    slices, _, _ = R.plain_slices(net.parsed)
    return all(torch.equal(bits(p.reshape(-1)), bits(net.plain[o:o + k])) for p, (o, k) in zip(net.model.parameters(), slices))


def test_adamw_step_without_attached_parameters():
    from g2048 import DeviceQNetwork
    net = device_net(random_model(2, 160, 2))
    boards, a, t, w = early_inputs(net.model)
    before, q_before = net.plain.clone(), net(boards).clone()
    assert not net.params_attached and net.opt_step == 0
    net.loss_and_grad(boards, a, t, w)
    norm = net.adamw_step(LR)
    assert norm.shape == () and norm.dtype == torch.float32 and float(norm) > 0
    assert net.opt_step == 1
    assert not torch.equal(net.plain, before) and module_is_plain(net)
    fresh = DeviceQNetwork(net.model)
    assert torch.equal(fresh.plain, net.plain) and torch.equal(fresh.packed, net.packed), "the blob was not packed again"
    assert torch.equal(net(boards), fresh(boards)) and not torch.equal(net(boards), q_before)
    assert net.exp_avg.any() and net.exp_avg_sq.any() and net.exp_avg.data_ptr() == net.exp_avg.data_ptr()
    # a bf16 network has no gradient path and is refused; step= overrides the count used, never the count kept
    with pytest.raises(ValueError, match="bf16.*refused"):
        DeviceQNetwork(net.model, precision="bf16").adamw_step(LR)
    net.adamw_step(LR, step=7)
    assert net.opt_step == 2 and module_is_plain(net)


def test_adamw_step_with_attached_parameters():
    """Measured on an MI355X: forward_batch after two device updates 1.37e-7 of max|Q| = 0.88 x the CPU-f32 error (bound 8 x)."""
    from g2048 import qnet
    net = device_net(random_model(2, 160, 2))
    boards, a, t, w = early_inputs(net.model)
    values = net.plain.clone()
    assert net.attach_params() is net.plain and net.params_attached
    assert torch.equal(net.plain, values), "attach_params changed the weights"
    slices, eps_at, _ = R.plain_slices(net.parsed)
    attached = lambda: all(p.data_ptr() == net.plain.data_ptr() + 4 * o and p.is_contiguous() for p, (o, _) in zip(net.model.parameters(), slices))
    assert attached()
    q0 = net.forward_batch(boards).clone()
    for step in (1, 2):                                     # no refresh() in between
        net.loss_and_grad(boards, a, t, w)
        net.adamw_step(LR)
        assert attached() and net.opt_step == step and module_is_plain(net)
    q = net.forward_batch(boards)
    assert not torch.equal(q, q0)
    m32 = copy.deepcopy(net.model).cpu().float()
    with torch.no_grad():
        f32 = m32(R.tile_values(boards.cpu().numpy(), torch.float32)).numpy().astype(np.float64)
    want = qnet.forward_batch_reference(qnet.parse(copy.deepcopy(m32).double()), boards.cpu()).numpy()
    check_q(q.cpu().numpy(), want, f32, "forward_batch after two attached updates")
    packed = net.packed.clone()
    assert not torch.equal(net(boards), device_net(random_model(2, 160, 2))(boards))
    # load_state_dict writes through into plain; refresh() then only packs
    other = random_model(5, 160, 2)
    net.model.load_state_dict(other.state_dict())
    assert attached() and torch.equal(net.plain[eps_at].cpu(), values[eps_at].cpu())
    assert torch.equal(net.plain.cpu(), qnet.flatten(qnet.parse(other)))
    net.refresh()
    assert not torch.equal(net.packed, packed) and torch.equal(net(boards), device_net(other)(boards))
    # new storage for the parameters undoes the attachment, and refresh() flattens again
    net.model.double().float()
    assert not net.params_attached
    net.refresh()
    assert torch.equal(net.plain.cpu(), qnet.flatten(qnet.parse(other)))


def test_sync_from_copies_the_online_network():
    online, target = device_net(random_model(2, 32, 1)), device_net(random_model(3, 32, 1))
    boards, a, t, w = early_inputs(online.model)
    assert not torch.equal(target.forward_batch(boards), online.forward_batch(boards))
    assert target.sync_from(online) is target
    assert torch.equal(bits(target.plain), bits(online.plain))
    assert torch.equal(target.forward_batch(boards), online.forward_batch(boards)) and torch.equal(target(boards), online(boards))
    assert module_is_plain(target)
    assert all(torch.equal(p, q) for p, q in zip(target.model.parameters(), online.model.parameters()))
    kept, q_kept = target.plain.clone(), target.forward_batch(boards).clone()
    online.loss_and_grad(boards, a, t, w)
    online.adamw_step(LR)
    assert torch.equal(target.plain, kept) and torch.equal(target.forward_batch(boards), q_kept), "the target followed the online network's step"
    assert not torch.equal(online.plain, kept)
    # an attached target takes the copy as its module; a bf16 target packs at its own precision
    target.attach_params()
    target.sync_from(online)
    assert target.params_attached and module_is_plain(target) and torch.equal(target.plain, online.plain)
    from g2048 import DeviceQNetwork
    half = DeviceQNetwork(copy.deepcopy(target.model), precision="bf16")
    half.sync_from(device_net(random_model(4, 32, 1)))
    assert torch.equal(half(boards), DeviceQNetwork(half.model, precision="bf16")(boards)) and half.packed.numel() < online.packed.numel()
    with pytest.raises(ValueError, match="dim_ff 64"):
        target.sync_from(device_net(random_model(2, 64, 1)))
    with pytest.raises(ValueError, match="2 layers"):
        target.sync_from(device_net(random_model(2, 32, 2)))
    with pytest.raises(TypeError, match="expected a DeviceQNetwork"):
        target.sync_from(online.model)


def mirror_step(model, optimizer, weights, grads, max_norm, lr):
    """One isolated step of a CPU mirror: its parameters := the device's pre-step weights, its gradients := the device's UNCLIPPED
    gradients, then its own clip_grad_norm_ and AdamW step at `lr` (its moment estimates are its own)."""
    with torch.no_grad():
        for p, w, g in zip(model.parameters(), weights, grads):
            p.copy_(torch.from_numpy(w).reshape(p.shape).to(p.dtype))
            p.grad = torch.from_numpy(g).reshape(p.shape).to(p.dtype)
    torch.nn.utils.clip_grad_norm_(list(model.parameters()), max_norm=max_norm)
    for group in optimizer.param_groups:
        group["lr"] = lr
    optimizer.step()
    return [p.detach().numpy().astype(np.float64).reshape(-1) for p in model.parameters()]


def test_closed_loop_of_three_rounds():
    """test_closed_loop_of_four_rounds with the tail on the device: adamw_step(cosine_lr(round)) for clip_grad_norm_ + AdamW +
    CosineAnnealingLR + refresh(), sync_from after round 1 for load_state_dict + refresh(). The online network's parameters are
    not attached (every round's CPU copies are taken from its module, so they see a step only if adamw_step loaded it back), the
    target's are. Measured on an MI355X (rounds 0 - 2): gradients 0.61, 0.61, 0.56 x the float32 copy's error, the optimiser
    step 1.00 x the float32 mirror's deviation in every round (7.8e-8 .. 7.9e-8 of max|w|; bound 8 x both); clipping acted in rounds
    0 and 1 (norms 7.54 and 6.42 against max_norm 3.77) and not in 2 (1.88)."""
    import g2048
    online, target = device_net(random_model(ONLINE_SEED, DIM_FF, LAYERS)), device_net(random_model(TARGET_SEED, DIM_FF, LAYERS))
    target.attach_params()
    buf = g2048.DeviceReplayBuffer(CAPACITY, alpha=0.6, device=DEV, seed=1)
    states, actions, rewards, nxt, dones = transitions()
    buf.push(*to_dev(states, actions, rewards, nxt, dones))
    mirrors = []
    for dtype in (torch.float64, torch.float32):
        m = copy.deepcopy(online.model).cpu().to(dtype)
        mirrors.append((m, torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=WEIGHT_DECAY)))
    slices, eps_at, _ = R.plain_slices(online.parsed)
    eps_plain = online.plain[eps_at].clone()
    max_norm, probe = None, None

    for rnd, u in enumerate(draws()[:3]):
        what = "round %d" % rnd
        on, tg = cpu_copies(online), cpu_copies(target)
        (_, acts, _, _, done_f), indices, weights, shaped = buf.sample(BATCH, beta=beta_of(rnd), u=to_dev(u)[0])
        boards, next_boards = buf.boards(indices)
        idx = indices.cpu().numpy()
        if probe is None:
            probe = boards.clone()
        targets, next_actions = g2048.dqn_targets(online, target, next_boards, shaped, done_f, GAMMA)
        t_np, w_np = targets.cpu().numpy(), weights.cpu().numpy()
        check_targets(what, t_np, next_actions.cpu().numpy(), shaped.cpu().numpy(), done_f.cpu().numpy(), on, tg, nxt[idx])

        loss, td, _ = online.loss_and_grad(boards, acts, targets, weights)
        want, f32 = (R.stock_loss_grad(m, states[idx], acts.cpu().numpy(), t_np, w_np) for m in on)
        grads, eps = split(online, online.grad)
        assert np.all(eps == 0), what
        check((float(loss), td.cpu().numpy().astype(np.float64), None, grads), want, f32, True, what)

        # ---- clipping and the optimiser step, on the device, against the CPU mirrors doing their own clipping
        if max_norm is None:
            max_norm = 0.5 * float(np.sqrt(sum(np.sum(g * g) for g in want[3])))
        lr = g2048.cosine_lr(rnd)
        norm64 = float(np.sqrt(sum(np.sum(g * g) for g in grads)))
        pre = [p.detach().numpy().astype(np.float64).reshape(-1) for p in on[1].parameters()]
        norm = float(online.adamw_step(lr, max_norm=max_norm, weight_decay=WEIGHT_DECAY))
        assert online.opt_step == rnd + 1
        print("%s: gradient norm %.4g, max_norm %.4g: clipping %s" % (what, norm, max_norm, "acted" if norm > max_norm else "did not act"))
        assert abs(norm - norm64) <= 1e-6 * norm64, (what, norm, norm64)
        assert rnd > 0 or norm > max_norm, "clipping must act in round 0"
        after = float(online.grad.double().norm())
        assert abs(after - min(norm, max_norm)) <= 1e-5 * min(norm, max_norm), (what, after, norm, max_norm)
        assert np.all(split(online, online.grad)[1] == 0), "%s: clipping moved a LayerNorm-eps slot of grad" % what
        post = [p.detach().cpu().numpy().astype(np.float64).reshape(-1) for p in online.model.parameters()]
        s64, s32 = (mirror_step(m, opt, pre, grads, max_norm, lr) for m, opt in mirrors)
        top = max(np.abs(x).max() for x in s64)
        e_dev, e_f32 = (max(np.abs(x - y).max() for x, y in zip(s, s64)) / top for s in (post, s32))
        moved = max(np.abs(x - y).max() for x, y in zip(post, pre))
        print("%s: optimiser step: weights moved by up to %.3g; device %.3g of max|w| from the float64 mirror = %.2f x the float32 "
              "mirror's %.3g (bound %.0f x)" % (what, moved, e_dev, e_dev / e_f32, e_f32, F32_FACTOR))
        assert 0.5e-3 < moved < 1.5e-3, what
        assert e_f32 > 0 and e_dev <= F32_FACTOR * e_f32, what
        assert module_is_plain(online) and torch.equal(online.plain[eps_at], eps_plain), what

        buf.update_priorities(indices, td)

        # ---- the target network
        if rnd == 1:
            assert not torch.equal(target.forward_batch(probe), online.forward_batch(probe)), "the target equals the online network before the sync"
            target.sync_from(online)
            assert torch.equal(target.plain, online.plain) and module_is_plain(target) and target.params_attached
            assert torch.equal(target.forward_batch(probe), online.forward_batch(probe)), "a synchronised target is not bit-equal to the online network"
        if rnd == 2:
            assert not torch.equal(target.forward_batch(probe), online.forward_batch(probe)), "the target followed the online network's step"


def test_example_trains_with_the_device_step():
    """test_example_trains with --device-step: the only place outside this file where attach_params, adamw_step and sync_from run in
    sequence with the buffer and the environments."""
    out = subprocess.run([sys.executable, os.path.join(REPO, "examples", "dqn_replay.py"), "--envs", "256", "--steps", "40", "--train",
                          "--device-step", "--dim-ff", "160"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rounds = re.search(r"with (\d+) sample \+ update rounds", out.stdout)
    loss = re.search(r"last weighted Huber loss (\S+)", out.stdout)
    norm = re.search(r"device step: (\d+) updates, last gradient norm before clipping (\S+)", out.stdout)
    assert rounds and int(rounds.group(1)) == 10 and loss and norm, out.stdout[-2000:]
    assert np.isfinite(float(loss.group(1))) and float(loss.group(1)) >= 0, out.stdout[-2000:]
    assert int(norm.group(1)) == 12 and np.isfinite(float(norm.group(2))) and float(norm.group(2)) > 0, out.stdout[-2000:]     # 2 warm-up rounds + 10
    without = subprocess.run([sys.executable, os.path.join(REPO, "examples", "dqn_replay.py"), "--device-step"], capture_output=True, text=True, timeout=300)
    assert without.returncode != 0 and "--device-step needs --train" in without.stderr
