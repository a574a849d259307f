"""g2048_ppo_adam_step on the MI355X: the NaN gate on the loss, gradient clipping and Adam over the actor's and the critic's plain
buffers in two launches, and DevicePPOLearner.adam_step / update / optimizer_state_dict / load_optimizer_state_dict around it.

The problem size is fixed by the two networks (46,532 and 46,337 floats; the critic's buffers end in a 16-byte group of ONE float).
The kernel is checked against the yardstick ppo_step_ref.adam_step_reference (itself clip_grad_norm_ + torch.optim.Adam to 1e-12:
tests/test_ppo_step_host.py). Tolerance, the convention of tests/test_gpu_qnet_step.py: per buffer max|device - y64| / max|y64| <=
8 x the same measure of the float32 yardstick, both yardsticks fed the device's own pre-step state; the float32 deviation must be
> 0. A norm is held to 1e-6 of the float64 norm of the device's gradient, a clipped gradient to 4 float32 ulps an element of grad . c
with c formed in float64 from the device's own norm, an unclipped one to its bits.

Measured on an MI355X: see the docstrings of the tests and docs/LOG.md R25."""
import contextlib
import copy
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import ppo_step_ref as S
import ppo_update_ref as R
from conftest import REPO
from test_gpu_ppo_update import DEV, check_running, learner_of, split_running, to_dev

pytestmark = pytest.mark.gpu

CANARY = 64
NAN, INF = float("nan"), float("inf")
KW = dict(lr=S.LR, eps=S.EPS, max_norm=S.MAX_NORM, betas=S.BETAS)
NAMES = ("plain", "grad", "exp_avg", "exp_avg_sq")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@contextlib.contextmanager
def no_sync():
    """Inside, a torch operation that synchronises with the host raises."""
    torch.cuda.synchronize()
    with warnings.catch_warnings():                      # torch says that the mode is a prototype
        warnings.simplefilter("ignore")
        torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


class Canaried:
    """The eight buffers (actor's plain, grad, exp_avg, exp_avg_sq, then the critic's), the norms, the counters and the workspace as
    slices of larger device tensors filled with 7: 64 floats before and after each buffer, the offsets multiples of 4 floats. The
    weights start as the case's, the moments and counters as zeros."""

    def __init__(self):
        from g2048 import ops
        plains, _ = S.step_case()
        sizes = [S.FLOATS[0]] * 4 + [S.FLOATS[1]] * 4
        self.whole = [torch.full((n + 2 * CANARY,), 7.0, device=DEV) for n in sizes]
        self.buffers = [w[CANARY:CANARY + n] for w, n in zip(self.whole, sizes)]
        self.norms_whole = torch.full((4,), 7.0, device=DEV)
        self.norms = self.norms_whole[1:3]
        self.counters_whole = torch.full((6,), 7, dtype=torch.int64, device=DEV)
        self.counters = self.counters_whole[1:5]
        self.nb = ops.ppo_step_workspace_bytes()
        self.workspace = torch.full((self.nb + 4096,), 7, dtype=torch.uint8, device=DEV)
        assert all(b.data_ptr() % 16 == 0 for b in self.buffers) and self.counters.data_ptr() % 8 == 0
        for k in (0, 1):
            self.buffers[4 * k].copy_(plains[k])
            self.buffers[4 * k + 2].zero_()
            self.buffers[4 * k + 3].zero_()
        self.counters.zero_()

    def net(self, k):
        return self.buffers[4 * k:4 * k + 4]

    def set_grads(self, grads):
        for k in (0, 1):
            self.buffers[4 * k + 1].copy_(grads[k])

    def set_moments(self, grads):
        """Moments as a few steps would leave them: exp_avg = 0.1 x a gradient, exp_avg_sq = the square of another."""
        for k in (0, 1):
            self.buffers[4 * k + 2].copy_(grads[1][k] * 0.1)
            self.buffers[4 * k + 3].copy_(grads[2][k] * grads[2][k])

    def pre(self):
        return [t.cpu().clone() for t in self.buffers]

    def step(self, losses=None, **kw):
        from g2048 import ops
        out = ops.ppo_adam_step(*self.buffers, self.counters, losses=losses, norms=self.norms, workspace=self.workspace, **dict(KW, **kw))
        assert out is self.norms
        return out

    def check(self, what):
        seven = bits(torch.tensor([7.0]))
        for w, b in zip(self.whole, self.buffers):
            assert torch.all(bits(w[:CANARY]) == seven) and torch.all(bits(w[CANARY + b.numel():]) == seven), \
                "%s: a canary next to a buffer was overwritten" % what
        assert self.norms_whole[0] == 7.0 and self.norms_whole[3] == 7.0, "%s: a canary next to the norms was overwritten" % what
        assert self.counters_whole[0] == 7 and self.counters_whole[5] == 7, "%s: a canary next to the counters was overwritten" % what
        assert torch.all(self.workspace[self.nb:] == 7), "%s: the workspace was written past its stated size" % what


def check_norm(norm, grad_pre, what):
    norm64 = float(np.linalg.norm(grad_pre.numpy().astype(np.float64)))
    assert abs(float(norm) - norm64) <= 1e-6 * norm64, (what, float(norm), norm64)
    return norm64


def check_network(pre, post, k, step, what, lr=S.LR, eps=S.EPS):
    """One network's post-step buffers against both yardsticks run from its pre-step buffers: the bound on weights and moments, and
    the gradient left behind. Returns the three multiples of the float32 yardstick's deviation."""
    y64, y32 = S.yardsticks(pre, k, step, lr=lr, eps=eps)
    row = []
    for i in (0, 2, 3):
        e_dev, e_f32 = S.deviation(post[i].numpy(), y64[i]), S.deviation(y32[i], y64[i])
        row.append(e_dev / e_f32 if e_f32 > 0 else np.inf)
        print("%s: %s %.3g of the largest entry from the float64 yardstick = %.2f x the float32 yardstick's %.3g (bound %.0f x)"
              % (what, NAMES[i], e_dev, row[-1], e_f32, S.F32_FACTOR))
        assert e_f32 > 0 and e_dev <= S.F32_FACTOR * e_f32, (what, NAMES[i])
    # printed, not asserted: the C-ABI takes lr as a float, so lr / bc1 is formed from (double)(float)lr
    y32f = S.yardsticks(pre, k, step, lr=tuple(float(np.float32(v)) for v in lr), eps=eps)[1]
    got = post[0].numpy().astype(np.float64)
    print("%s: plain differs from the float32 yardstick in %d elements, from the float32 yardstick with lr rounded to float32 first in %d"
          % (what, np.count_nonzero(got != y32[0]), np.count_nonzero(got != y32f[0])))
    return row


def check_clipped_gradient(norm, g_pre, g_post, clipped, what):
    coef = S.clip_coefficient(float(norm))
    assert (coef < 1.0) == clipped, (what, coef)
    g_pre, g_post = g_pre.numpy(), g_post.numpy()
    if coef == 1.0:
        assert np.array_equal(g_post.view(np.int32), g_pre.view(np.int32)), "%s: an unclipped gradient changed" % what
        return
    want = g_pre.astype(np.float64) * coef
    ulps = np.abs(g_post.astype(np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    print("%s: clipped gradient within %.2f float32 ulps of grad . c (c = %.9g)" % (what, ulps.max(), coef))
    assert ulps.max() <= 4.0, what


def run_steps(verify):
    """The four steps through ops.ppo_adam_step on canaried slices; returns the bits of the eight buffers at the end, of every step's
    norms and the multiples measured."""
    _, grads = S.step_case()
    c = Canaried()
    norms, ratios = [], []
    for s in range(4):
        c.set_grads(grads[s])
        pre = c.pre()
        c.step()
        norms.append(bits(c.norms).clone())
        if not verify:
            continue
        c.check("step %d" % (s + 1))
        post = c.pre()
        for k, name in enumerate(("actor", "critic")):
            what = "step %d, %s" % (s + 1, name)
            norm64 = check_norm(c.norms[k], pre[4 * k + 1], what)
            assert norm64 == pytest.approx(S.FACTORS[k][s] * S.MAX_NORM, rel=1e-6)
            ratios.append(check_network(pre[4 * k:4 * k + 4], post[4 * k:4 * k + 4], k, s + 1, what))
            check_clipped_gradient(c.norms[k], pre[4 * k + 1], post[4 * k + 1], S.FACTORS[k][s] >= 1.0, what)
        if s == 0:          # the critic's last float, a 16-byte group of its own: fc4.bias took a first Adam step of about lr
            moved = abs(float(post[4][-1].double() - pre[4][-1].double()))
            assert 0.5 * S.LR[1] < moved < 1.5 * S.LR[1], moved
    assert c.counters.tolist() == [4, 4, 0, 0]
    return [bits(t).clone() for t in c.buffers], norms, ratios


def test_four_steps_against_the_yardstick_with_canaries_and_bit_for_bit_twice():
    """The actor's norm runs 2, 1, 0.5, 0.5 x max_norm and the critic's 0.5, 2, 1, 0.5 x: step 1 clips the actor alone, step 2 both (the
    actor at its edge), step 3 the critic alone, at its edge, step 4 neither; lr and eps differ per network. Measured on an MI355X,
    all four steps and both networks: weights, exp_avg and exp_avg_sq each 1.00 x the float32 yardstick's deviation from the float64
    one (weights 3.1e-8 .. 3.3e-8 of max|w|, moments 1.5e-8 .. 1.5e-7; bound 8 x); the clipped gradients within 1.25 float32 ulps of
    grad . c at c = 0.4999995 and 0.94 at c = 0.999998, bit-equal at c = 1; the second run bit-equal in all eight buffers and the
    norms. adam_step takes 30.5 us against the stock tail's 405 us (profiles/r25_ppo_step_rate.txt)."""
    first, norms, ratios = run_steps(verify=True)
    again, norms_again, _ = run_steps(verify=False)
    assert all(torch.equal(a, b) for a, b in zip(first, again)), "two runs from the same state differ in a buffer"
    assert all(torch.equal(a, b) for a, b in zip(norms, norms_again)), "two runs from the same state differ in a norm"
    print("worst multiple of the float32 yardstick's deviation %.2f" % max(max(r) for r in ratios))


@pytest.mark.parametrize("value, net, where", [(INF, 0, 1), (NAN, 0, 23001), (-INF, 1, 23002), (NAN, 1, -1)],
                         ids=["inf-actor-first-group", "nan-actor-middle", "-inf-critic-middle", "nan-critic-last-float"])
def test_a_gradient_that_is_not_finite_changes_nothing_in_either_network(value, net, where):
    """All eight buffers keep their bits, the norm of the network without the bad element is finite and right, the step counters
    stay and counters[3] counts the call."""
    _, grads = S.step_case()
    c = Canaried()
    c.set_grads(grads[0])
    c.set_moments(grads)
    c.counters.copy_(torch.tensor([3, 3, 1, 2]))
    c.buffers[4 * net + 1][where] = value
    pre, pre_bits = c.pre(), [bits(t).clone() for t in c.buffers]
    norms = c.step(losses=torch.zeros(4, device=DEV))
    assert not np.isfinite(float(norms[net]))
    check_norm(norms[1 - net], pre[4 * (1 - net) + 1], "the other network")
    assert all(torch.equal(a, bits(b)) for a, b in zip(pre_bits, c.buffers)), "a buffer changed although a norm is not finite"
    assert c.counters.tolist() == [3, 3, 1, 3]
    c.check("not finite")


def gate_call(losses):
    """One call from the same start (moments as after a few steps, counters {5, 2, 0, 0}: the networks' step numbers differ): (pre
    buffers, post buffers, norms bits, counters, the Canaried)."""
    _, grads = S.step_case()
    c = Canaried()
    c.set_grads(grads[0])
    c.set_moments(grads)
    c.counters.copy_(torch.tensor([5, 2, 0, 0]))
    pre = c.pre()
    c.step(losses=None if losses is None else torch.tensor(losses, dtype=torch.float32, device=DEV))
    c.check("loss gate")
    return pre, c.pre(), bits(c.norms).clone(), c.counters.tolist(), c


def test_the_loss_gate():
    """losses=None is applied (each network at ITS step number, 6 and 3); a NaN loss[0] over finite gradients changes nothing and
    counts in counters[2], the norms still written; loss[0] = +inf is applied (isnan only, the reference's rule); a NaN in loss[1..3]
    with a finite loss[0] is applied. The applied calls give the ungated call's bits. Measured on an MI355X: the actor at step 6
    1.00 x the float32 yardstick's deviation on all three buffers, the critic at step 3 2.34 x on the weights (5.4e-8 of max|w|) and
    1.00 x on the moments. The 2.34 x is lr's: the C-ABI takes it as a float, and with lr rounded to float32 first the float32
    yardstick's weights differ from the device's in 531 elements instead of 2,851 (check_network prints both counts)."""
    pre, base, norms, counters, _ = gate_call(None)
    assert counters == [6, 3, 0, 0]
    for k, name in enumerate(("actor", "critic")):
        check_network(pre[4 * k:4 * k + 4], base[4 * k:4 * k + 4], k, (6, 3)[k], "losses=None, %s at step %d" % (name, (6, 3)[k]))
    same = lambda a, b: all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))      # noqa: E731

    _, post, norms_nan, counters, _ = gate_call([NAN, 1.0, 1.0, 1.0])
    assert same(post, pre), "a NaN loss changed a buffer"
    assert counters == [5, 2, 1, 0] and torch.equal(norms_nan, norms)

    for what, losses in (("+inf loss", [INF, 1.0, 1.0, 1.0]), ("-inf loss", [-INF, 1.0, 1.0, 1.0]), ("NaN in loss[1..3]", [0.25, NAN, NAN, NAN]),
                         ("a finite loss", [0.25, 0.1, 0.3, 1.2])):
        _, post, norms_k, counters, _ = gate_call(losses)
        assert same(post, base), "%s: not the ungated call's bits" % what
        assert counters == [6, 3, 0, 0] and torch.equal(norms_k, norms), what


def test_the_step_number_is_the_devices():
    """apply, skip (NaN loss), apply: the third call is Adam step 2 of both networks and meets the bound against the yardstick at step
    2. tests/test_ppo_step_host.py asserts that the yardstick at step 3 is more than twice the bound away, so counting the skipped
    call cannot pass."""
    _, grads = S.step_case()
    c = Canaried()
    c.set_grads(grads[0])
    c.step(losses=torch.tensor([0.5, 0, 0, 0], dtype=torch.float32, device=DEV))
    c.set_grads(grads[1])
    held = [bits(t).clone() for t in c.buffers]
    c.step(losses=torch.tensor([NAN, 0, 0, 0], dtype=torch.float32, device=DEV))
    assert all(torch.equal(a, bits(b)) for a, b in zip(held, c.buffers)) and c.counters.tolist() == [1, 1, 1, 0]
    pre = c.pre()
    c.step(losses=torch.tensor([0.5, 0, 0, 0], dtype=torch.float32, device=DEV))
    post = c.pre()
    assert c.counters.tolist() == [2, 2, 1, 0]
    for k, name in enumerate(("actor", "critic")):
        check_network(pre[4 * k:4 * k + 4], post[4 * k:4 * k + 4], k, 2, "apply, skip, apply: %s against step 2" % name)
    c.check("apply, skip, apply")


def test_a_late_step():
    """The counters loaded with 100,000 (actor) and 100,000 // 7 (critic): one call against the yardstick at t + 1. At 14,286 the second
    bias correction is still 6e-7 away from 1, ten float32 ulps."""
    _, grads = S.step_case()
    c = Canaried()
    c.set_grads(grads[0])
    c.set_moments(grads)
    t = (100000, 100000 // 7)
    c.counters.copy_(torch.tensor([t[0], t[1], 0, 0]))
    pre = c.pre()
    c.step()
    post = c.pre()
    assert c.counters.tolist() == [t[0] + 1, t[1] + 1, 0, 0]
    for k, name in enumerate(("actor", "critic")):
        check_network(pre[4 * k:4 * k + 4], post[4 * k:4 * k + 4], k, t[k] + 1, "late step, %s at %d" % (name, t[k] + 1))
    c.check("late step")


# ------------------------------------------------------------------------------------------------------ the learner --
LOOP_KW = dict(lr=(R.LR_ACTOR, R.LR_CRITIC), eps=(R.LR_ACTOR, R.LR_CRITIC), max_norm=R.MAX_NORM)


def learner_bits(learner):
    return [t.clone() for net in (learner.actor, learner.critic) for t in (net.plain, net.grad, net.running, net.exp_avg, net.exp_avg_sq)] + \
           [learner.opt_counters.clone()]


def device_loop(c):
    """tests/test_gpu_ppo_update_edges.py's device_loop with learner.adam_step(losses) for the stock clip and Adam."""
    learner, actor, critic = learner_of(c.nets32)
    learner.attach_params()
    x, nx, rewards, dones = to_dev(*c.inputs)
    actions, old = to_dev(c.actions, c.old)
    params = [p for m in (actor, critic) for p in m.parameters()]
    start = [p.detach().cpu().numpy().astype(np.float64).reshape(-1) for p in params]
    ret, adv = learner.advantages(x, nx, rewards, dones)
    out = dict(returns=ret.cpu().numpy().astype(np.float64), advantages=adv.cpu().numpy().astype(np.float64), epochs=[])
    for _ in range(R.LOOP_EPOCHS):
        losses = learner.loss_and_grad(x, actions, old, adv, ret)
        ep = dict(losses=losses.cpu().numpy().astype(np.float64), loss_bits=bits(losses).clone())
        ep["norms64"] = tuple(float(np.linalg.norm(net.grad.cpu().numpy().astype(np.float64))) for net in (learner.actor, learner.critic))
        norms = learner.adam_step(losses, **LOOP_KW)
        assert norms.shape == (2,) and norms.dtype == torch.float32 and norms.is_cuda
        ep["norms"], ep["norm_bits"] = tuple(norms.tolist()), bits(norms).clone()
        ep["delta"] = [p.detach().cpu().numpy().astype(np.float64).reshape(-1) - s for p, s in zip(params, start)]
        out["epochs"].append(ep)
    torch.cuda.synchronize()
    out["bits"] = learner_bits(learner)
    out["views_held"] = all(torch.equal(net.plain[o:o + p.numel()], p.detach().reshape(-1))
                            for net, m in ((learner.actor, actor), (learner.critic, critic)) for p, (_, o, _) in zip(m.parameters(), net.offsets))
    out["running"] = split_running(learner.actor.running) + split_running(learner.critic.running)
    out["tracked"] = [int(bn.num_batches_tracked) for m in (actor, critic) for bn in (m.bn1, m.bn2)]
    out["counters"] = learner.opt_counters.tolist()
    return out


def test_whole_update_three_epochs_on_the_device():
    """test_whole_update_three_epochs_closed_loop with adam_step for the stock tail, under that test's bounds: per epoch the loss parts
    within the case's bound, each tensor's accumulated change p_e - p_0 off from float64's by at most 8 x the float32 run's deviation
    (never tighter than 2^-23 max|p|); running statistics within the bound, num_batches_tracked 3, 3, 5, 5, the buffers equal to the
    modules' parameters bit for bit; the norms within 1e-6 of the device gradient's float64 norms. Then learner.update(epochs=3) from
    the same start, with torch's synchronisation check set to raise: the same bits in plain, grad, running, the moments and the
    counters, and losses and norms rows that are the manual sequence's bits. Measured on an MI355X: loss parts 0.02 x the yardstick
    in every epoch, parameter changes at most 0.13 / 0.15 / 0.14 of their bound, running statistics 0.33 x; update(epochs=8) at n = 256
    takes 1,425 us against 4,434 us with the stock tail (profiles/r25_ppo_step_rate.txt)."""
    c = R.loop_case()
    got = device_loop(c)
    assert max(R.rel(got["returns"], c.want["adv"]["returns"]), R.rel(got["advantages"], c.want["adv"]["advantages"])) <= c.adv_bound
    for e, (g, w, f) in enumerate(zip(got["epochs"], c.want["epochs"], c.f32["epochs"])):
        e_loss = R.rel(g["losses"], w["losses"])
        worst, where = 0.0, -1
        for k, (dg, dw, df, s) in enumerate(zip(g["delta"], w["delta"], f["delta"], c.want["start"])):
            err, mirror = np.abs(dg - dw).max(), np.abs(df - dw).max()
            tol = max(R.F32_FACTOR * mirror, 2.0 ** -23 * np.abs(s).max())
            if err / tol > worst:
                worst, where = err / tol, k
        print("epoch %d: loss parts %.2f x the yardstick %.3g; gradient norms %.3g / %.3g (float64 %.3g / %.3g); parameter changes at most "
              "%.2f of their bound (tensor %d)" % (e, e_loss / c.yardstick, c.yardstick, g["norms"][0], g["norms"][1], w["norms"][0],
                                                   w["norms"][1], worst, where))
        assert np.isfinite(g["losses"]).all() and e_loss <= c.bound
        assert worst <= 1.0, "epoch %d, tensor %d: p_e - p_0 is off by %.2f of its bound" % (e, where, worst)
        for k in (0, 1):
            assert abs(g["norms"][k] - g["norms64"][k]) <= 1e-6 * g["norms64"][k], (e, k, g["norms"][k], g["norms64"][k])
    check_running(c, got["running"], c.want["running"], "after %d epochs" % R.LOOP_EPOCHS)
    assert got["tracked"] == [3, 3, 5, 5] == c.want["tracked"]
    assert got["views_held"], "a plain buffer no longer equals its module's parameters"
    assert got["counters"] == [3, 3, 0, 0]

    learner, actor, critic = learner_of(c.nets32)
    learner.attach_params()
    x, nx, rewards, dones = to_dev(*c.inputs)
    actions, old = to_dev(c.actions, c.old)
    torch.cuda.synchronize()
    with no_sync():
        losses, norms = learner.update(x, actions, old, rewards, nx, dones, epochs=R.LOOP_EPOCHS, **LOOP_KW)
    torch.cuda.synchronize()
    assert losses.shape == (R.LOOP_EPOCHS, 4) and norms.shape == (R.LOOP_EPOCHS, 2) and losses.is_cuda and norms.is_cuda
    assert all(torch.equal(a, b) for a, b in zip(got["bits"], learner_bits(learner))), "update() and the manual sequence leave other bits"
    for e, ep in enumerate(got["epochs"]):
        assert torch.equal(bits(losses[e]), ep["loss_bits"]) and torch.equal(bits(norms[e]), ep["norm_bits"]), "epoch %d" % e
    assert [int(bn.num_batches_tracked) for m in (actor, critic) for bn in (m.bn1, m.bn2)] == [3, 3, 5, 5]
    with pytest.raises(TypeError, match="unexpected arguments"):
        learner.update(x, actions, old, rewards, nx, dones, epochs=1, weight_decay=0.1)
    with pytest.raises(ValueError, match="at least one epoch"):
        learner.update(x, actions, old, rewards, nx, dones, epochs=0)


def stepped_learner(steps, attach=True):
    """A learner on the case's modules after the given steps' gradients through adam_step."""
    _, grads = S.step_case()
    learner, actor, critic = learner_of(R.make_modules())
    if attach:
        learner.attach_params()
    for s in steps:
        set_learner_grads(learner, grads[s])
        learner.adam_step(None, **KW)
    return learner, actor, critic


def set_learner_grads(learner, grads):
    learner.actor.grad.copy_(grads[0])
    learner.critic.grad.copy_(grads[1])


def net_buffers(net):
    return [t.cpu().clone() for t in (net.plain, net.grad, net.exp_avg, net.exp_avg_sq)]


def test_checkpoint_interop_with_torch_optim_adam():
    """After two device steps optimizer_state_dict(which) loads into a fresh torch.optim.Adam over a float64 deep copy of the module;
    its third step (stock clip_grad_norm_ + step) and the device's third step agree within the bound. The other way: a stock float32
    optimizer's state after two stock steps, loaded into a fresh learner, continues on the device as step 3."""
    _, grads = S.step_case()
    learner, actor, critic = stepped_learner((0, 1))
    assert learner.optimizer_state_dict("actor")["state"][0]["step"] == 2 and learner.opt_counters.tolist() == [2, 2, 0, 0]
    with pytest.raises(ValueError, match="'actor' or 'critic'"):
        learner.optimizer_state_dict("both")
    stock = []
    for k, (which, module) in enumerate((("actor", actor), ("critic", critic))):
        sd = learner.optimizer_state_dict(which)
        assert sorted(sd["state"]) == list(range(12)) and sd["param_groups"][0]["params"] == list(range(12))
        assert sd["param_groups"][0]["lr"] == S.LR[k] and sd["param_groups"][0]["eps"] == S.EPS[k]
        m64 = copy.deepcopy(module).cpu().double()
        opt = torch.optim.Adam(m64.parameters(), lr=123.0)
        opt.load_state_dict(sd)
        stock.append((m64, opt))
    set_learner_grads(learner, grads[2])
    pre = [net_buffers(net) for net in (learner.actor, learner.critic)]
    learner.adam_step(None, **KW)
    post = [net_buffers(net) for net in (learner.actor, learner.critic)]
    for k, (m64, opt) in enumerate(stock):
        params, o = list(m64.parameters()), 0
        for p in params:
            p.grad = grads[2][k][o:o + p.numel()].double().view(p.shape).clone()
            o += p.numel()
        torch.nn.utils.clip_grad_norm_(params, S.MAX_NORM)
        opt.step()
        flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).numpy()      # noqa: E731
        want = (flat(params), None, flat([opt.state[p]["exp_avg"] for p in params]), flat([opt.state[p]["exp_avg_sq"] for p in params]))
        assert all(int(opt.state[p]["step"]) == 3 for p in params)
        _, y32 = S.yardsticks(pre[k], k, 3)
        for i in (0, 2, 3):
            e_dev, e_f32 = S.deviation(post[k][i].numpy(), want[i]), S.deviation(y32[i], want[i])
            print("third step, %s %s: device %.3g of the largest entry from the stock float64 optimizer = %.2f x the float32 yardstick's %.3g"
                  % (("actor", "critic")[k], NAMES[i], e_dev, e_dev / e_f32, e_f32))
            assert e_f32 > 0 and e_dev <= S.F32_FACTOR * e_f32

    # the other way
    modules = [copy.deepcopy(m) for m in R.make_modules()]
    opts = [torch.optim.Adam(m.parameters(), lr=S.LR[k], eps=S.EPS[k]) for k, m in enumerate(modules)]
    for s in (0, 1):
        for k, (m, opt) in enumerate(zip(modules, opts)):
            o = 0
            for p in m.parameters():
                p.grad = grads[s][k][o:o + p.numel()].view(p.shape).clone()
                o += p.numel()
            torch.nn.utils.clip_grad_norm_(m.parameters(), S.MAX_NORM)
            opt.step()
    fresh, _, _ = learner_of(modules)
    fresh.attach_params()
    for which, opt in zip(("actor", "critic"), opts):
        fresh.load_optimizer_state_dict(which, opt.state_dict())
    assert fresh.opt_counters.tolist() == [2, 2, 0, 0]
    for net, m, opt in zip((fresh.actor, fresh.critic), modules, opts):
        assert torch.equal(net.exp_avg.cpu(), torch.cat([opt.state[p]["exp_avg"].reshape(-1) for p in m.parameters()]))
        assert torch.equal(net.exp_avg_sq.cpu(), torch.cat([opt.state[p]["exp_avg_sq"].reshape(-1) for p in m.parameters()]))
    set_learner_grads(fresh, grads[2])
    pre = [net_buffers(net) for net in (fresh.actor, fresh.critic)]
    fresh.adam_step(None, **KW)
    for k, net in enumerate((fresh.actor, fresh.critic)):
        check_network(pre[k], net_buffers(net), k, 3, "continued from a stock optimizer's state, %s" % ("actor", "critic")[k])
    assert fresh.opt_counters.tolist() == [3, 3, 0, 0]
    # a fresh optimizer's (empty) state resets; a state of another shape is refused
    fresh.load_optimizer_state_dict("critic", torch.optim.Adam(modules[1].parameters()).state_dict())
    assert fresh.opt_counters.tolist() == [3, 0, 0, 0] and not fresh.critic.exp_avg.any() and not fresh.critic.exp_avg_sq.any()
    with pytest.raises(ValueError, match="shape"):
        fresh.load_optimizer_state_dict("critic", opts[0].state_dict())
    assert learner.optimizer_state_dict("actor")["state"][11]["exp_avg"].shape == (4,) and fresh.optimizer_state_dict("critic")["state"] == {}


def test_unattached_learner_ends_with_write_back():
    """Without attach_params() the modules' parameters keep their own storage, and after adam_step they equal the plain buffers bit for
    bit, and the attached learner's. The call runs with torch's synchronisation check set to raise: write_back() must not wait
    for the device either."""
    loose, actor, critic = learner_of(R.make_modules())
    ptrs = [p.data_ptr() for m in (actor, critic) for p in m.parameters()]
    before = [p.detach().clone() for m in (actor, critic) for p in m.parameters()]
    _, grads = S.step_case()
    set_learner_grads(loose, grads[0])
    with no_sync():                                      # write_back()'s 32 copies included
        loose.adam_step(torch.zeros(4, device=DEV), **KW)
    attached, a_actor, a_critic = stepped_learner((0,))
    assert ptrs == [p.data_ptr() for m in (actor, critic) for p in m.parameters()] and not loose.actor.params_attached
    assert attached.actor.params_attached and attached.critic.params_attached
    for net, m, other in ((loose.actor, actor, a_actor), (loose.critic, critic, a_critic)):
        for p, q, (name, o, _) in zip(m.parameters(), other.parameters(), net.offsets):
            assert torch.equal(bits(net.plain[o:o + p.numel()]), bits(p.reshape(-1))), name
            assert torch.equal(bits(p), bits(q)), name
    assert all(not torch.equal(p, b) for p, b in zip([p for m in (actor, critic) for p in m.parameters()], before))
    assert torch.equal(loose.actor.plain, attached.actor.plain) and torch.equal(loose.critic.plain, attached.critic.plain)


def test_side_stream_gives_the_same_bits_in_other_buffers():
    """adam_step inside torch.cuda.stream(side) from the same state: the default stream's bits in all eight buffers and the counters,
    the norms in a buffer of the side stream's own; the default stream's norms buffer is not written."""
    _, grads = S.step_case()
    learner, _, _ = stepped_learner((0,))
    set_learner_grads(learner, grads[1])
    state = learner_bits(learner)
    with no_sync():                                      # adam_step on its own, the parameters attached
        norms = learner.adam_step(None, **KW)
    torch.cuda.synchronize()
    want, want_norms = learner_bits(learner), norms.clone()
    for t, s in zip(learner_bits_live(learner), state):
        t.copy_(s)
    norms.fill_(7.0)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        norms_side = learner.adam_step(None, **KW)
    side.synchronize()
    torch.cuda.current_stream(DEV).wait_stream(side)
    assert norms_side.data_ptr() != norms.data_ptr() and bool(torch.all(norms == 7.0))
    assert torch.equal(bits(norms_side), bits(want_norms))
    assert all(torch.equal(a, b) for a, b in zip(learner_bits(learner), want))
    assert learner.opt_counters.tolist() == [2, 2, 0, 0]


def learner_bits_live(learner):
    return [t for net in (learner.actor, learner.critic) for t in (net.plain, net.grad, net.running, net.exp_avg, net.exp_avg_sq)] + \
           [learner.opt_counters]


def test_example_updates_with_the_device_optimizer():
    """examples/ppo_rollout.py --learner device --optimizer device: the epoch loop as one learner.update() call; the device-update line
    keeps its format and its loss is finite. --optimizer device without --learner device is refused."""
    script = os.path.join(REPO, "examples", "ppo_rollout.py")
    out = subprocess.run([sys.executable, script, "--envs", "1024", "--steps", "16", "--learner", "device", "--optimizer", "device"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = re.search(r"device update on 256 sampled transitions \(of 16384\): loss (\S+) \(actor (\S+), value (\S+), entropy (\S+)\) after 8 epochs",
                     out.stdout)
    assert line and all(np.isfinite(float(v)) for v in line.groups()), out.stdout[-2000:]
    counts = re.search(r"device optimizer: (\d+) / (\d+) Adam steps applied \(actor / critic\), (\d+) epochs skipped for a NaN loss, (\d+) for",
                       out.stdout)
    assert counts and [int(v) for v in counts.groups()] == [8, 8, 0, 0], out.stdout[-2000:]
    without = subprocess.run([sys.executable, script, "--optimizer", "device"], capture_output=True, text=True, timeout=300)
    assert without.returncode != 0 and "--optimizer device needs --learner device" in without.stderr
