"""The PPO update's loss and gradient pass (csrc/g2048_ppo_grad.hip, g2048.DevicePPOLearner) on the MI355X away from the one regime
of tests/test_gpu_ppo_update.py: non-finite inputs, which must show in the loss and the gradients as they do in stock torch;
DevicePPOLearner.advantages() end to end and the advantages block at a zero deviation; a saturated policy (logits that span more than
float32's exp, probabilities that round to exactly 1); coefficients other than the reference agent's, 0 among them; a whole update of
three epochs with stock clipping and Adam on the views against the same sequence on the stock float64 modules; the learner without
attach_params() / attach_grads() and on a side stream; features that are 0 on every row. The cases are built by
tests/ppo_update_ref.py and their conditions asserted on the CPU by tests/test_ppo_update_host.py.

Tolerance: the case's bound of tests/test_gpu_ppo_update.py throughout (8 x stock CPU float32 autograd's own worst tensor against
float64); where a test needs another measure its docstring derives it. Every measured multiple is printed; docs/LOG.md R24 has them."""
import copy
import warnings

import numpy as np
import pytest
import torch

import ppo_update_ref as R
from test_gpu_ppo_update import CANARY, DEV, Call, check_case, check_running, learner_of, split, split_running, to_dev

pytestmark = pytest.mark.gpu


def quiet_update(nets, args, **kw):
    with warnings.catch_warnings():                      # NumPy and torch warn about the NaN they are asked to produce
        warnings.simplefilter("ignore")
        return R.stock_update(nets, *args, **kw)


class Front:
    """What check_case reads, taken from a learner after loss_and_grad."""

    def __init__(self, learner, losses):
        torch.cuda.synchronize()
        self.grads = split(learner.actor, learner.actor.grad) + split(learner.critic, learner.critic.grad)
        self.losses = losses.cpu().numpy().astype(np.float64)
        self.bits = [learner.actor.grad.clone(), learner.critic.grad.clone(), losses.clone()]


# ------------------------------------------------------------------------------------------------ non-finite inputs --
@pytest.mark.parametrize("poison", R.POISONS, ids=[p[0] for p in R.POISONS])
@pytest.mark.parametrize("n", R.POISON_SIZES)
def test_non_finite_input_shows_as_in_stock_torch(n, poison):
    """One non-finite value in the last row of old_log_probs, advantages or returns (at n = 129 the first row of the head's third
    block). Stock CPU float32 on the same inputs gives the pattern: each loss part is finite, NaN, +inf or -inf as stock's is, and
    each of the 24 gradient tensors holds a non-finite value exactly when stock's does. The network the poison does not reach keeps
    every gradient finite and within the case's bound of float64, and so do the loss parts that stay finite (one tensor, relative
    to the largest of them). old_log_probs = +inf is ratio = 0 and everything finite: the ordinary bound on all tensors. Inside a
    poisoned network's tensors the element-wise agreement of the finite masks is printed, not asserted (0 x NaN in a product)."""
    name, which, value, sign, clean = poison
    c = R.case(n)
    args = R.poisoned_args(c, which, value, sign)
    f32, f64 = quiet_update(c.nets32, args), quiet_update(c.nets64, args)
    learner, _, _ = learner_of(c.nets32)
    got = Call(learner, c, None, None, None, CANARY, args=args)
    assert got.canaries_intact(CANARY)
    print("n = %d, %s: loss parts %s (stock float32 %s)" % (n, name, R.classes(got.losses), R.classes(f32["losses"])))
    assert R.classes(got.losses) == R.classes(f32["losses"]), "a loss part's class differs from stock float32's"
    assert R.nonfinite(got.grads) == R.nonfinite(f32["grads"]), "a gradient tensor is finite where stock's is not, or the reverse"
    keep = slice(12, 24) if clean == "critic" else slice(0, 12)
    assert not any(R.nonfinite(got.grads[keep]))
    r = R.ratios(got.grads[keep], f64["grads"][keep])
    finite = [k for k, cl in enumerate(R.classes(f32["losses"])) if cl == "finite"]
    e_loss = np.abs(got.losses[finite] - f64["losses"][finite]).max() / np.abs(f64["losses"][finite]).max()
    print("  the %s's gradients %.2f x the yardstick, the finite loss parts %s %.2f x" % (clean, r.max() / c.yardstick, finite, e_loss / c.yardstick))
    assert r.max() <= c.bound and e_loss <= c.bound
    if name == "old=+inf":
        check_case(c, got, "n = %d, %s" % (n, name), f64)
    else:
        other = slice(0, 12) if clean == "critic" else slice(12, 24)
        same = [float(np.mean(np.isfinite(g) == np.isfinite(w))) for g, w in zip(got.grads[other], f32["grads"][other])]
        print("  element-wise agreement of the finite masks with stock float32, per tensor: %s" % " ".join("%.3f" % v for v in same))


@pytest.mark.parametrize("n", R.POISON_SIZES)
def test_nan_state_is_reported_in_the_loss(n):
    """A NaN in one row of `states`: stock Categorical refuses NaN probabilities, so there is no torch pattern; the loss must be NaN,
    reported and not hidden (every ReLU of the training pass passes a NaN on, as torch.relu does)."""
    c = R.case(n)
    x = c.x.copy()
    x[-1, 3] = np.nan
    learner, _, _ = learner_of(c.nets32)
    got = Call(learner, c, None, None, None, CANARY, args=(x,) + c.args[1:])
    print("n = %d, NaN state: loss parts %s" % (n, R.classes(got.losses)))
    assert np.isnan(got.losses[0])


def test_advantages_block_nan_reward_and_zero_deviation():
    """The advantages block at n = 17. A NaN reward: the finite masks of returns and advantages are stock float32 torch's on
    ppo_agent.py:368-373 (the row's return, every advantage). All advantages equal (rewards 1, values 0.25, next values 0, every
    float32 step exact): the deviation is 0 and the divisor 1e-8; stock float32 torch gives returns 1 and advantages exactly 0, and
    relative to a maximum of 0 the bound admits only 0: the outputs equal torch's, all finite."""
    from g2048 import ops
    n = 17
    rng = np.random.default_rng(57)
    values, next_values = rng.normal(0, 2, n).astype(np.float32), rng.normal(0, 2, n).astype(np.float32)
    rewards = rng.normal(1, 3, n).astype(np.float32)
    rewards[5] = np.nan
    dones = (np.arange(n) % 3 == 1).astype(np.float32)
    want = R.advantage_lines(torch.float32, values, next_values, rewards, dones)
    got = [t.cpu().numpy() for t in ops.ppo_advantages(*to_dev(values, next_values, rewards, dones), 0.995)]
    for g, w, what in zip(got, want, ("returns", "advantages")):
        assert np.array_equal(np.isfinite(g), np.isfinite(w)) and np.array_equal(np.isnan(g), np.isnan(w)), what
    finite = np.isfinite(want[0])
    assert R.rel(got[0][finite].astype(np.float64), want[0][finite]) <= R.F32_FACTOR * R.ADV_FLOOR

    flat = (np.full(n, 0.25, np.float32), np.zeros(n, np.float32), np.ones(n, np.float32), np.zeros(n, np.float32))
    want, f64 = R.advantage_lines(torch.float32, *flat), R.advantage_lines(torch.float64, *flat)
    bound = R.advantage_bound(want, f64)
    got = [t.cpu().numpy().astype(np.float64) for t in ops.ppo_advantages(*to_dev(*flat), 0.995)]
    e = [R.rel(g, w) for g, w in zip(got, want)]
    print("advantages, zero deviation: returns %.3g, advantages %.3g against stock float32 (bound %.3g)" % (e[0], e[1], bound))
    assert all(np.isfinite(g).all() for g in got) and max(e) <= bound and not got[1].any()


# ----------------------------------------------------------------------------------------- advantages() end to end --
def test_learner_advantages_end_to_end():
    """DevicePPOLearner.advantages() at n = 48 (the closed-loop case's inputs) against ppo_agent.py:357-373 on the stock float64
    critic in training mode: returns and advantages within 8 x stock float32's own error (at least 8 x 8 x 2^-24, the floor of the
    advantages block's test), the critic's running statistics after its two forwards within the same bound, num_batches_tracked
    + 2 on the critic's BatchNorms and + 0 on the actor's. The two forwards' outputs are different buffers holding the values of
    `states` and of `next_states`; the advantages are those of returns - values(states), recomputed from a separate values() call.
    The results are cache-owned, as documented: a second call with other inputs returns the same storage, now holding its own
    results (checked against float64 too), and a clone of the first call's is what keeps them."""
    from g2048 import ppo
    c = R.loop_case()
    learner, actor, critic = learner_of(c.nets32)
    learner.attach_params()
    x, nx, rewards, dones = to_dev(*c.inputs)
    actor_running = learner.actor.running.clone()
    ret, adv = learner.advantages(x, nx, rewards, dones)
    torch.cuda.synchronize()
    kept = ret.clone(), adv.clone()
    want = c.want["adv"]
    got = [t.cpu().numpy().astype(np.float64) for t in kept]
    e = R.rel(got[0], want["returns"]), R.rel(got[1], want["advantages"])
    print("advantages() n = %d: returns %.3g, advantages %.3g of their maxima (bound %.3g)" % (R.LOOP_N, e[0], e[1], c.adv_bound))
    assert max(e) <= c.adv_bound
    r = R.ratios(split_running(learner.critic.running), c.want["running_adv"][4:])
    print("  the critic's running statistics after the two forwards %.3g of their maxima" % r.max())
    assert r.max() <= c.adv_bound
    assert torch.equal(learner.actor.running, actor_running) and torch.equal(critic.bn1.running_mean, learner.critic.running[:256])
    assert [int(bn.num_batches_tracked) for bn in (critic.bn1, critic.bn2, actor.bn1, actor.bn2)] == [2, 2, 0, 0]

    v_buf, nv_buf = learner._out.get(R.LOOP_N, ppo._values), learner._out.get(R.LOOP_N, ppo._next_values)
    assert v_buf.data_ptr() != nv_buf.data_ptr()
    assert R.rel(v_buf.cpu().numpy().reshape(-1), want["values"]) <= c.adv_bound
    assert R.rel(nv_buf.cpu().numpy().reshape(-1), want["next_values"]) <= c.adv_bound
    values = learner.values(x).cpu().numpy().astype(np.float64).reshape(-1)
    a = got[0] - values
    a = (a - a.mean()) / (a.std(ddof=1) + 1e-8)
    assert R.rel(got[1], a) <= c.adv_bound, "the advantages are not returns - values(states), normalised"

    i = np.arange(R.LOOP_N)
    rewards2, dones2 = (c.inputs[2][::-1] + 1.0).astype(np.float32), (i % 4 == 1).astype(np.float32)
    ret2, adv2 = learner.advantages(nx, x, *to_dev(rewards2, dones2))
    torch.cuda.synchronize()
    assert ret2.data_ptr() == ret.data_ptr() and adv2.data_ptr() == adv.data_ptr()      # cache-owned: the docstring's word
    assert not torch.equal(ret, kept[0]) and not torch.equal(adv, kept[1])
    f64, f32 = (R.stock_advantages(copy.deepcopy(net[1]), c.inputs[1], c.inputs[0], rewards2, dones2) for net in (c.nets64, c.nets32))
    pair = lambda d: (d["returns"].numpy().astype(np.float64), d["advantages"].numpy().astype(np.float64))       # noqa: E731
    bound2 = R.advantage_bound(pair(f32), pair(f64))
    assert max(R.rel(ret2.cpu().numpy(), pair(f64)[0]), R.rel(adv2.cpu().numpy(), pair(f64)[1])) <= bound2
    assert R.rel(kept[0].cpu().numpy(), want["returns"]) == e[0] and R.rel(kept[1].cpu().numpy(), want["advantages"]) == e[1]


# --------------------------------------------------------------------------------------------------- saturated policy --
def test_saturated_policy():
    """The actor's fc4.weight x 128 at n = 32: logit gaps up to 167, so softmax must subtract the maximum; on 22 rows float32's q is
    exactly 1 and the upper clamp binds, the other actions are clamped from below, and rows differ in which. All 24 gradients and
    the loss parts against float64 evaluated with float32's eps (in float32 that evaluation is torch's bit for bit,
    tests/test_ppo_update_host.py), the loss parts against stock float32 as well, forward_train's probabilities against float64;
    every output finite, and the device's q is exactly 1 on the rows the CPU test calls saturated and on no other."""
    from g2048 import ops
    c = R.saturated_case()
    learner, _, _ = learner_of(c.nets32)
    probs = ops.ppo_forward_train(to_dev(c.x)[0], learner.actor.plain, 4).cpu().numpy().astype(np.float64)
    sat = R.saturated_measures(c.nets64, c.x)["rest"] < R.SAT_LOW
    e = R.rel(probs, c.want["probs"])
    print("saturated case: forward_train probabilities %.3g of max = %.2f x the yardstick %.3g" % (e, e / c.yardstick, c.yardstick))
    assert np.isfinite(probs).all() and e <= c.bound
    assert np.array_equal(probs.max(1) == 1.0, sat)
    got = Call(learner, c, None, None, None, CANARY)
    assert got.canaries_intact(CANARY)
    e = R.rel(got.losses, c.f32["losses"])
    print("saturated case: loss parts %.3g of their maximum against stock float32 = %.2f x the yardstick" % (e, e / c.yardstick))
    assert e <= c.bound
    check_case(c, got, "saturated case, float64 with float32's eps")


# ------------------------------------------------------------------------------------------------------- coefficients --
@pytest.mark.parametrize("k", range(len(R.COEF_SETS)), ids=["clip%g-value%g-entropy%g" % s for s in R.COEF_SETS])
def test_other_coefficients(k):
    """(clip, value_coef, entropy_coef) other than the reference agent's, through DevicePPOLearner's own arguments, against float64
    autograd with the same coefficients. value_coef = 0: every critic gradient exactly 0. entropy_coef = 0: the loss is
    actor + value_coef x value of the device's own parts, to float32 rounding (2^-23 of the largest part)."""
    c = R.coef_case(k)
    clip, value_coef, entropy_coef = c.coefs
    learner, _, _ = learner_of(c.nets32, clip_epsilon=clip, value_coef=value_coef, entropy_coef=entropy_coef)
    got = Front(learner, learner.loss_and_grad(*to_dev(*c.args)))
    check_case(c, got, "coefficients %s" % (c.coefs,))
    if value_coef == 0.0:
        assert all(not g.any() for g in got.grads[12:]), "value_coef = 0 left a critic gradient that is not exactly 0"
    if entropy_coef == 0.0:
        own = got.losses[1] + value_coef * got.losses[2]
        assert abs(got.losses[0] - own) <= 2.0 ** -23 * np.abs(got.losses).max()


# ------------------------------------------------------------------------------------------------------ dead features --
def test_dead_features_at_a_real_batch_size():
    """fc1.bias = -10 on features 0 - 7 of both modules at n = 17: the features are 0 on every row, BatchNorm's variance there is 0
    and its output its bias. The usual bound on all tensors; exactly 0 in fc1.weight's rows, fc1.bias and bn1.weight at every dead
    feature (those eight and the ones this seed leaves dead by itself, R.DEAD_ACTOR / R.DEAD_CRITIC); bn1.bias there within the
    bound and not 0, fc2.weight's columns there not 0 (BatchNorm's output is beta)."""
    c = R.dead_case()
    learner, _, _ = learner_of(c.nets32)
    got = Call(learner, c, None, None, None, CANARY)
    check_case(c, got, "dead features")
    for dead, base, net in ((R.DEAD_ACTOR, 0, "actor"), (R.DEAD_CRITIC, 12, "critic")):
        idx, g = list(dead), got.grads
        assert not g[base + 0].reshape(256, 16)[idx].any(), "%s: fc1.weight has a gradient on a dead feature" % net
        assert not g[base + 1][idx].any() and not g[base + 2][idx].any(), "%s: fc1.bias or bn1.weight has a gradient on a dead feature" % net
        assert np.abs(g[base + 3][idx]).min() > 0 and np.abs(g[base + 4].reshape(128, 256)[:, idx]).max(0).min() > 0, net
        assert np.abs(c.want["grads"][base + 3][idx]).min() > 0


# ----------------------------------------------------------------------------------------------------- a whole update --
def device_loop(c):
    """PPOAgent.update()'s sequence on an attached DevicePPOLearner: advantages(), then per epoch loss_and_grad, stock
    clip_grad_norm_(0.5) and a stock Adam step (eps = lr) per module on the views."""
    learner, actor, critic = learner_of(c.nets32)
    learner.attach_params()
    learner.attach_grads()
    opts = (torch.optim.Adam(actor.parameters(), lr=R.LR_ACTOR, eps=R.LR_ACTOR), torch.optim.Adam(critic.parameters(), lr=R.LR_CRITIC, eps=R.LR_CRITIC))
    x, nx, rewards, dones = to_dev(*c.inputs)
    actions, old = to_dev(c.actions, c.old)
    params = [p for m in (actor, critic) for p in m.parameters()]
    start = [p.detach().cpu().numpy().astype(np.float64).reshape(-1) for p in params]
    ret, adv = learner.advantages(x, nx, rewards, dones)
    out = dict(returns=ret.cpu().numpy().astype(np.float64), advantages=adv.cpu().numpy().astype(np.float64), epochs=[])
    for _ in range(R.LOOP_EPOCHS):
        losses = learner.loss_and_grad(x, actions, old, adv, ret)
        ep = dict(losses=losses.cpu().numpy().astype(np.float64))
        ep["norms"] = tuple(float(torch.nn.utils.clip_grad_norm_(m.parameters(), R.MAX_NORM)) for m in (actor, critic))
        for opt in opts:
            opt.step()
        ep["delta"] = [p.detach().cpu().numpy().astype(np.float64).reshape(-1) - s for p, s in zip(params, start)]
        out["epochs"].append(ep)
    torch.cuda.synchronize()
    out["bits"] = [t.clone() for net in (learner.actor, learner.critic) for t in (net.plain, net.grad, net.running)]
    out["views_held"] = all(torch.equal(net.plain[o:o + p.numel()], p.detach().reshape(-1))
                            for net, m in ((learner.actor, actor), (learner.critic, critic)) for p, (_, o, _) in zip(m.parameters(), net.offsets))
    out["running"] = split_running(learner.actor.running) + split_running(learner.critic.running)
    out["tracked"] = [int(bn.num_batches_tracked) for m in (actor, critic) for bn in (m.bn1, m.bn2)]
    return out


def test_whole_update_three_epochs_closed_loop():
    """n = 48, three epochs of update()'s own sequence, three runs: the device learner, the stock float64 modules (the reference)
    and the stock float32 modules (the measure). Adam's eps is its lr, for the reason in test_front_end_attached_adam_step_and_
    policy_refresh: at 1e-8 a gradient within rounding of zero moves a weight by 2 lr in stock float32 too. Per epoch the loss
    parts within the case's bound, and for each of the 24 parameter tensors the accumulated change p_e - p_0 off from float64's by at
    most 8 x the float32 run's deviation for that tensor, and never held tighter than the rounding of the stored weight, 2^-23 max|p|.
    After the last epoch: running statistics within the bound, num_batches_tracked 3 (actor) and 5 (critic), the plain buffers
    equal to the modules' parameters bit for bit, and a second run from the same start the same bits in plain, grad and running."""
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
    check_running(c, got["running"], c.want["running"], "after %d epochs" % R.LOOP_EPOCHS)
    assert got["tracked"] == [3, 3, 5, 5] == c.want["tracked"]
    assert got["views_held"], "a plain buffer no longer equals its module's parameters"
    again = device_loop(c)
    assert all(torch.equal(a, b) for a, b in zip(got["bits"], again["bits"])), "a second run from the same start gives other bits"


# ------------------------------------------------------------------------------- unattached learner, a side stream --
def test_unattached_learner_refresh_and_write_back():
    """Without attach_params() / attach_grads() at n = 16: loss_and_grad leaves the modules' parameters, .grad and running buffers
    untouched; learner.actor.grad / learner.critic.grad hold the gradients, the same bits as an attached learner's on the same
    inputs (and within the bound of float64); write_back() makes the modules equal to changed plain and running buffers,
    refresh() the buffers equal to changed modules."""
    c = R.case(16)
    args = to_dev(*c.args)
    learner, actor, critic = learner_of(c.nets32)
    state = [copy.deepcopy(m.state_dict()) for m in (actor, critic)]
    ptrs = [p.data_ptr() for m in (actor, critic) for p in m.parameters()]
    got = Front(learner, learner.loss_and_grad(*args))
    check_case(c, got, "unattached learner, n = 16")
    for m, sd in zip((actor, critic), state):
        for key, t in m.state_dict().items():
            if not key.endswith("num_batches_tracked"):
                assert torch.equal(t, sd[key]), key
        assert all(p.grad is None for p in m.parameters())
    assert ptrs == [p.data_ptr() for m in (actor, critic) for p in m.parameters()]
    assert not torch.equal(learner.actor.running[:256], actor.bn1.running_mean)          # the buffer moved, the module's did not
    attached, _, _ = learner_of(c.nets32)
    attached.attach_params()
    attached.attach_grads()
    other = Front(attached, attached.loss_and_grad(*args))
    assert all(torch.equal(a, b) for a, b in zip(got.bits, other.bits))

    with torch.no_grad():
        for net in (learner.actor, learner.critic):
            net.plain.mul_(1.5).add_(0.125)
            net.running.mul_(0.5).add_(1.0)
    learner.write_back()

    def buffers_equal_modules():
        from g2048 import ops
        for net, m in ((learner.actor, actor), (learner.critic, critic)):
            for p, (name, o, _) in zip(m.parameters(), net.offsets):
                assert torch.equal(net.plain[o:o + p.numel()], p.detach().reshape(-1)), name
            for t, (name, o, k) in zip((m.bn1.running_mean, m.bn1.running_var, m.bn2.running_mean, m.bn2.running_var), ops.PPO_RUNNING_OFFSETS):
                assert torch.equal(net.running[o:o + k], t), name
    buffers_equal_modules()
    assert not torch.equal(actor.fc1.weight, state[0]["fc1.weight"]) and not torch.equal(critic.bn2.running_var, state[1]["bn2.running_var"])
    with torch.no_grad():
        for m in (actor, critic):
            for p in m.parameters():
                p.mul_(-0.75)
            m.bn1.running_mean.add_(2.0)
            m.bn2.running_var.mul_(3.0)
    assert not torch.equal(learner.actor.plain[:4096], actor.fc1.weight.detach().reshape(-1))
    learner.refresh()
    buffers_equal_modules()


def test_side_stream_gives_the_same_bits_in_other_buffers():
    """One loss_and_grad and one advantages() at n = 16 inside torch.cuda.stream(side), the inputs made ready on that stream: the same
    bits as the default stream's, in output buffers distinct from the default stream's (OutputCache keys them by stream)."""
    c = R.case(16)
    nx = R.states_of(16, R.SEEDS[16] + 1)
    i = np.arange(16)
    rewards, dones = ((7 * i) % 5 - 2.0).astype(np.float32), (i % 3 == 1).astype(np.float32)
    learner, _, _ = learner_of(c.nets32)
    args = to_dev(*c.args)
    first = Front(learner, learner.loss_and_grad(*args))
    losses = learner.loss_and_grad(*args)
    ret, adv = learner.advantages(args[0], *to_dev(nx, rewards, dones))
    torch.cuda.synchronize()
    kept = [t.clone() for t in (losses, ret, adv)]
    learner.actor.grad.fill_(CANARY)
    learner.critic.grad.fill_(CANARY)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        args_side = to_dev(*c.args)
        rest_side = to_dev(nx, rewards, dones)
        losses_side = learner.loss_and_grad(*args_side)
        ret_side, adv_side = learner.advantages(args_side[0], *rest_side)
    side.synchronize()
    torch.cuda.current_stream(DEV).wait_stream(side)
    assert not {t.data_ptr() for t in (losses_side, ret_side, adv_side)} & {t.data_ptr() for t in (losses, ret, adv)}
    for a, b in zip((losses_side, ret_side, adv_side), kept):
        assert torch.equal(a, b)
    for a, b in zip((losses, ret, adv), kept):                      # the default stream's buffers were not written
        assert torch.equal(a, b)
    assert torch.equal(learner.actor.grad, first.bits[0]) and torch.equal(learner.critic.grad, first.bits[1])
