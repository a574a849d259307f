"""g2048_ppo_loss_grad, g2048_ppo_forward_train and g2048_ppo_advantages on the MI355X: the four loss parts, all 24 gradient
tensors, the training-mode forwards and the moved running statistics against the stock modules' CPU float64 autograd through
agents/ppo_agent.py:378-400 (tests/ppo_update_ref.py) at n = 1 (BatchNorm skipped), the tile edges, the eight-tile group of the dW
product, the reference's batch of 256 and the batch limit, with canaries, repeatability and a poisoned workspace; the advantages
block against float64 torch; a case in which Categorical's clamp binds; the front end with a stock Adam on the views and
DevicePolicy.refresh(); and the gradients of the reference's own classes (tests/golden/ppo_update.npz).

Tolerance, the convention of tests/qnet_grad_ref.py per case: for every gradient tensor max|g - g64| / max|g64| <= 8 x the worst
such ratio of stock CPU float32 autograd over the case's 24 tensors (the case's yardstick); the loss parts (one tensor of four),
the probabilities, the values and each running statistic are held to the same bound relative to their own maxima. The inputs'
conditions (ReLU margins, a fair float32 yardstick, no probability near the clamp, no ratio at a clip edge) are asserted on the CPU
by tests/test_ppo_update_host.py. The measured multiples are printed.

The four loss parts are ONE tensor, held relative to the largest of them: the total is a difference of the parts (0.01 .. 0.3 where the
value loss is about 1), and its error relative to itself (printed, up to 1.5e-5 at n = 4,096) is the cancellation's, in stock float32
too.

Measured on an MI355X (per case in docs/LOG.md R23.1): gradients 0.27 - 2.28 x the case's yardstick (7.2e-7 .. 2.9e-6 at n >= 15,
4.4e-5 at n = 2, 4.8e-6 at n = 3, 3.6e-7 at n = 1 on the test machine's CPU), the worst at n = 3 (critic fc2.bias) and 1.64 x at
n = 17; loss parts <= 0.16 x; probabilities <= 0.26 x, values <= 0.43 x (1.54 x at n = 1, where the yardstick is 3.6e-7); running
statistics <= 0.14 x after one call and <= 0.36 x after three; the clamp case 0.61 x (loss parts against stock float32 0.11 x); the
reference classes' fixture 0.41 x of a yardstick of 1.6e-5; advantages <= 8.3e-8 of their maxima (bound 3.8e-6); the Adam step at most
0.12 of its derived tolerance. Added with docs/LOG.md R24.1: n = 31, 33, 224, 225 (the edges of BatchNorm's 32 row groups and its
passes of 256 rows; gradients 1.49, 2.35, 1.19, 1.88 x) and the advantages block at n = 255, 256, 257, 4,095 (<= 9.5e-8). The regimes
away from this one are in tests/test_gpu_ppo_update_edges.py."""
import copy

import numpy as np
import pytest
import torch

import ppo_update_ref as R
from conftest import load_golden
from test_ppo_update_host import golden_modules

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = 7.0
PAD = 64


def to_dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in arrays)


def learner_of(nets32, **kw):
    """A DevicePPOLearner on deep copies of the float32 modules, moved to the device."""
    from g2048 import DevicePPOLearner
    actor, critic = (copy.deepcopy(net).to(DEV) for net in nets32)
    return DevicePPOLearner(actor, critic, **kw), actor, critic


def padded(floats, fill=CANARY):
    """(buffer of floats + PAD, the view of the first `floats`)."""
    t = torch.full((floats + PAD,), fill, dtype=torch.float32, device=DEV)
    return t, t[:floats]


def split(learner_net, grad):
    g = grad.cpu().numpy().astype(np.float64)
    return [g[o:o + int(np.prod(shape))] for _, o, shape in learner_net.offsets]


def split_running(running):
    from g2048 import ops
    r = running.cpu().numpy().astype(np.float64)
    return [r[o:o + k] for _, o, k in ops.PPO_RUNNING_OFFSETS]


class Call:
    """One g2048_ppo_loss_grad call through ops into padded outputs; everything the checks need, as float64 NumPy plus the bits."""

    def __init__(self, learner, c, run_a, run_c, workspace, fill, args=None):
        from g2048 import ops
        clip, value_coef, entropy_coef = c.coefs
        self.ga_all, ga = padded(ops.ppo_plain_floats(4), fill)
        self.gc_all, gc = padded(ops.ppo_plain_floats(1), fill)
        self.l_all, losses = padded(4, fill)
        ops.ppo_loss_grad(*to_dev(*(c.args if args is None else args)), learner.actor.plain, learner.critic.plain, run_a, run_c, clip,
                          value_coef, entropy_coef, grad_actor=ga, grad_critic=gc, losses=losses, workspace=workspace)
        torch.cuda.synchronize()
        self.bits = [t.clone() for t in (ga, gc, losses)]
        self.grads = split(learner.actor, ga) + split(learner.critic, gc)
        self.losses = losses.cpu().numpy().astype(np.float64)

    def canaries_intact(self, fill):
        return all(bool(torch.all(t[-PAD:] == fill)) for t in (self.ga_all, self.gc_all, self.l_all))


def check_case(c, got, what, want=None):
    """The bound on the 24 gradients and the loss parts; returns (worst multiple of the yardstick, loss multiple)."""
    want = c.want if want is None else want
    r = R.ratios(got.grads, want["grads"])
    e_loss = R.rel(got.losses, want["losses"])
    worst = int(np.argmax(r))
    print("%s: gradients %.3g of max|g| (tensor %d) = %.2f x the CPU-f32 error %.3g (bound %.0f x); loss parts %.2f x (%s)"
          % (what, r[worst], worst, r[worst] / c.yardstick, c.yardstick, R.F32_FACTOR, e_loss / c.yardstick,
             " ".join("%.3g" % v for v in np.abs(got.losses - want["losses"]) / np.abs(want["losses"]))))
    assert all(np.all(np.isfinite(g)) for g in got.grads) and np.all(np.isfinite(got.losses)), what
    assert c.yardstick > 0 and r.max() <= c.bound, what
    assert e_loss <= c.bound, what
    return r[worst] / c.yardstick, e_loss / c.yardstick


def check_running(c, got, want, what):
    r = R.ratios(got, want)
    print("%s: running statistics %.3g of their maxima = %.2f x the yardstick" % (what, r.max(), r.max() / c.yardstick))
    assert r.max() <= c.bound, what


@pytest.mark.parametrize("n", R.GPU_SIZES)
def test_loss_grad_and_forward_train_against_float64(n):
    """Per n: all 24 gradient tensors, the four loss parts, forward_train's probabilities and values and the running statistics after
    one and after three calls against CPU float64; canaries after the end of both gradient buffers, of the losses, of the workspace
    and after row n of forward_train's outputs; three calls (the first on a workspace poisoned with NaN and outputs prefilled with
    another value) give identical bits; running = None gives the same bits and touches nothing. n = 1: the BatchNorm gradients are
    exactly 0 and the running statistics keep their bits."""
    from g2048 import ops
    c = R.case(n)
    learner, _, _ = learner_of(c.nets32)
    nb = ops.ppo_train_workspace_bytes(n)
    ws_all = torch.full((nb // 4 + PAD,), float("nan"), dtype=torch.float32, device=DEV)
    ws_all[nb // 4:] = CANARY
    ws = ws_all.view(torch.uint8)[:nb]
    run0 = (learner.actor.running.clone(), learner.critic.running.clone())
    run_a, run_c = run0[0].clone(), run0[1].clone()

    first = Call(learner, c, run_a, run_c, ws, CANARY)
    assert first.canaries_intact(CANARY) and bool(torch.all(ws_all[nb // 4:] == CANARY)), "written past the end of an output (n = %d)" % n
    check_case(c, first, "n = %d" % n)
    if n == 1:
        assert torch.equal(run_a, run0[0]) and torch.equal(run_c, run0[1]), "n = 1 moved the running statistics"
        assert all(not first.grads[k].any() for k in (2, 3, 6, 7, 14, 15, 18, 19)), "n = 1: a BatchNorm gradient is not exactly 0"
    else:
        assert not torch.equal(run_a, run0[0]) and not torch.equal(run_c, run0[1])
        check_running(c, split_running(run_a) + split_running(run_c), c.want["running"], "n = %d, one call" % n)
    after_one = (run_a.clone(), run_c.clone())

    for k in (2, 3):                              # the workspace as the last call left it, the outputs prefilled differently
        again = Call(learner, c, run_a, run_c, ws, -3.0)
        assert again.canaries_intact(-3.0)
        assert all(torch.equal(a, b) for a, b in zip(first.bits, again.bits)), "call %d differs from the first (n = %d)" % (k, n)
    if n > 1:
        check_running(c, split_running(run_a) + split_running(run_c), c.want_after(3)["running"], "n = %d, three calls" % n)
    kept = (run_a.clone(), run_c.clone())
    none = Call(learner, c, None, None, ws, CANARY)
    assert all(torch.equal(a, b) for a, b in zip(first.bits, none.bits)) and torch.equal(run_a, kept[0]) and torch.equal(run_c, kept[1])

    # forward_train, one network at a time, into outputs with rows to spare
    x = to_dev(c.x)[0]
    for net, key, run_before, run_after in ((learner.actor, "probs", run0[0], after_one[0]), (learner.critic, "values", run0[1], after_one[1])):
        out_all = torch.full((n + 9, net.n_out), CANARY, dtype=torch.float32, device=DEV)
        running = run_before.clone()
        ops.ppo_forward_train(x, net.plain, net.n_out, running=running, out=out_all[:n], workspace=ws)
        torch.cuda.synchronize()
        assert bool(torch.all(out_all[n:] == CANARY)), "rows past n were written (n = %d)" % n
        got = out_all[:n].cpu().numpy().astype(np.float64).reshape(c.want[key].shape)
        e = R.rel(got, c.want[key])
        print("n = %d: forward_train %s %.3g of max = %.2f x the yardstick" % (n, key, e, e / c.yardstick))
        assert e <= c.bound
        assert torch.equal(running, run_after), "forward_train and loss_grad move the running statistics differently"
        same = torch.full((n, net.n_out), CANARY, dtype=torch.float32, device=DEV)
        ops.ppo_forward_train(x, net.plain, net.n_out, running=None, out=same, workspace=ws)
        assert torch.equal(same, out_all[:n]) and bool(torch.all(ws_all[nb // 4:] == CANARY))


def test_batch_above_the_limit_is_refused():
    c = R.case(17)
    learner, _, _ = learner_of(c.nets32)
    n = 4097
    x = torch.zeros((n, 16), dtype=torch.float32, device=DEV)
    f = torch.zeros(n, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="refused, not truncated"):
        learner.loss_and_grad(x, torch.zeros(n, dtype=torch.int64, device=DEV), f, f, f)
    with pytest.raises(ValueError, match="refused, not truncated"):
        learner.values(x)
    with pytest.raises(ValueError, match="refused, not truncated"):
        learner.advantages(x, x, f, f)


@pytest.mark.parametrize("n", [1, 2, 17, 255, 256, 257, 4095, 4096])      # 255 .. 257: the edges of the block's 256-thread tree
def test_advantages_against_float64_torch(n):
    """ppo_agent.py:368-373 with dones of 0 and 1 against the same lines in float64 torch (no normalisation at n = 1). The bound:
    the inputs are float32 and the lines are a handful of float32 operations and two sums of n terms; stock float32 torch on the
    same lines is the measure, 8 x its error relative to the outputs' maxima (at least 8 float32 roundings, 8 x 2^-24)."""
    from g2048 import ops
    rng = np.random.default_rng(40 + n)
    values, next_values = rng.normal(0, 2, n).astype(np.float32), rng.normal(0, 2, n).astype(np.float32)
    rewards = rng.normal(1, 3, n).astype(np.float32)
    dones = (np.arange(n) % 3 == 1).astype(np.float32)
    if n > 1:
        assert set(dones.tolist()) == {0.0, 1.0}

    def lines(dtype):
        v, nv, r, d = (torch.from_numpy(t).to(dtype) for t in (values, next_values, rewards, dones))
        returns = r + 0.995 * nv * (1 - d)
        adv = returns - v
        if adv.shape[0] > 1:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        return returns.numpy().astype(np.float64), adv.numpy().astype(np.float64)
    want, f32 = lines(torch.float64), lines(torch.float32)
    bound = R.F32_FACTOR * max(R.rel(f32[0], want[0]), R.rel(f32[1], want[1]), 8 * 2.0 ** -24)
    ret_all = torch.full((n + 9,), CANARY, dtype=torch.float32, device=DEV)
    adv_all = torch.full((n + 9,), CANARY, dtype=torch.float32, device=DEV)
    ops.ppo_advantages(*to_dev(values.reshape(n, 1), next_values, rewards, dones), 0.995, returns=ret_all[:n], advantages=adv_all[:n])
    torch.cuda.synchronize()
    assert bool(torch.all(ret_all[n:] == CANARY)) and bool(torch.all(adv_all[n:] == CANARY))
    e = [R.rel(t[:n].cpu().numpy().astype(np.float64), w) for t, w in ((ret_all, want[0]), (adv_all, want[1]))]
    print("advantages n = %d: returns %.3g, advantages %.3g of their maxima (bound %.3g)" % (n, e[0], e[1], bound))
    assert max(e) <= bound
    again = ops.ppo_advantages(*to_dev(values, next_values, rewards, dones), 0.995)
    assert torch.equal(again[0], ret_all[:n]) and torch.equal(again[1], adv_all[:n])


def test_binding_clamp_against_stock_float32():
    """The actor's fc4.bias puts one action's probability below 1e-9 on every row and the even rows take it: Categorical clamps it
    to 2^-23 and passes no gradient. Stock CPU FLOAT32 autograd is the reference for the loss (float64 clamps at 2^-52): the loss parts
    within the case's bound of it, every gradient finite; the gradients are also held to the bound against the float64 evaluation with
    float32's eps (tests/test_ppo_update_host.py: in float32 that evaluation is torch's bit for bit)."""
    from g2048 import ops
    c = R.clamp_case()
    learner, _, _ = learner_of(c.nets32)
    probs = ops.ppo_forward_train(to_dev(c.x)[0], learner.actor.plain, 4)
    assert float(probs[:, R.CLAMP_ACTION].max()) < 1e-9
    got = Call(learner, c, None, None, None, CANARY)
    e = R.rel(got.losses, c.f32["losses"])
    print("clamp case: loss parts %.3g of their maximum against stock float32 = %.2f x the yardstick %.3g" % (e, e / c.yardstick, c.yardstick))
    assert e <= c.bound
    assert all(np.all(np.isfinite(g)) for g in got.grads)
    check_case(c, got, "clamp case, float64 with float32's eps")


def test_front_end_attached_adam_step_and_policy_refresh():
    """DevicePPOLearner end to end at n = 16: attach_params / attach_grads make the modules' tensors views of the buffers; probs,
    values and loss_and_grad agree with float64 and count num_batches_tracked; one stock Adam step on the views against the same
    step on the stock float64 modules driven by stock autograd; DevicePolicy.refresh() on the same modules, back in eval mode, then
    reproduces their eval forward.

    The step's bound: Adam's first step is lr . g / (|g| + eps), whose slope in g is at most lr / eps. At torch's default eps = 1e-8
    a gradient within rounding of zero moves a weight by 2 lr in stock float32 too, so the test takes lr = eps = 0.05: the step's
    error is then at most the gradient's, bound x max|g|, plus the float32 rounding of the updated weight (2^-23 max|p|) and of the
    step's own arithmetic (4 x 2^-23 max|step|)."""
    from g2048 import DevicePolicy
    lr = eps = 0.05
    c = R.case(16)
    learner, actor, critic = learner_of(c.nets32)
    policy = DevicePolicy(actor.eval(), critic.eval())
    actor.train(), critic.train()
    learner.attach_params()
    learner.attach_grads()
    for net, module in ((learner.actor, actor), (learner.critic, critic)):
        base, gbase = net.plain.data_ptr(), net.grad.data_ptr()
        for (name, p), (_, o, _) in zip(module.named_parameters(), net.offsets):
            assert p.data_ptr() == base + 4 * o and p.grad.data_ptr() == gbase + 4 * o, name
        assert module.bn1.running_var.data_ptr() == net.running.data_ptr() + 4 * 256
        assert module.bn2.running_mean.data_ptr() == net.running.data_ptr() + 4 * 512
    x = to_dev(c.x)[0]
    before = [t.clone() for t in (learner.actor.running, learner.critic.running)]
    p, v = learner.probs(x), learner.values(x)
    assert R.rel(p.cpu().numpy(), c.want["probs"]) <= c.bound and R.rel(v.cpu().numpy().reshape(-1), c.want["values"]) <= c.bound
    assert int(actor.bn1.num_batches_tracked) == 1 and int(critic.bn2.num_batches_tracked) == 1
    assert not torch.equal(actor.bn1.running_mean, before[0][:256])             # the module's buffer IS the moved one
    losses = learner.loss_and_grad(*to_dev(*c.args))
    assert losses.shape == (4,) and losses.is_cuda and int(actor.bn2.num_batches_tracked) == 2
    assert R.rel(losses.cpu().numpy(), c.want["losses"]) <= c.bound
    got = [p.grad.detach().cpu().numpy().astype(np.float64).reshape(-1) for m in (actor, critic) for p in m.parameters()]
    assert R.ratios(got, c.want["grads"]).max() <= c.bound

    # the same Adam step on the stock float64 modules, driven by stock autograd
    stock = [copy.deepcopy(net) for net in c.nets64]
    xs, a = torch.from_numpy(c.x).double(), torch.from_numpy(c.actions)
    old, adv, ret = (torch.from_numpy(t).double() for t in (c.old, c.adv, c.ret))
    lp, ent = R.categorical_parts(stock[0](xs), a)
    ratio = torch.exp(lp - old)
    loss = (-torch.min(ratio * adv, torch.clamp(ratio, 1 - R.CLIP, 1 + R.CLIP) * adv).mean()
            + R.VALUE_COEF * torch.nn.functional.mse_loss(stock[1](xs).squeeze(), ret) - R.ENTROPY_COEF * ent.mean())
    loss.backward()
    params = [p for m in (actor, critic) for p in m.parameters()]
    params64 = [p for m in stock for p in m.parameters()]
    old_p = [p.detach().cpu().numpy().astype(np.float64) for p in params]
    old_p64 = [p.detach().numpy().copy() for p in params64]
    torch.optim.Adam(params, lr=lr, eps=eps).step()
    torch.optim.Adam(params64, lr=lr, eps=eps).step()
    worst = 0.0
    for k, (p, p64, o, o64) in enumerate(zip(params, params64, old_p, old_p64)):
        step, step64 = p.detach().cpu().numpy().astype(np.float64) - o, p64.detach().numpy() - o64
        gmax, top = np.abs(c.want["grads"][k]).max(), np.abs(step64).max()
        tol = (lr / eps) * c.bound * gmax + 2.0 ** -23 * np.abs(o).max() + 4 * 2.0 ** -23 * top
        err = np.abs(step - step64).max()
        worst = max(worst, err / tol)
        assert top > 0 and err <= tol, "tensor %d: step error %.3g, tolerance %.3g (max|step| %.3g)" % (k, err, tol, top)
        # the optimiser wrote through the views
        net, j = (learner.actor, k) if k < 12 else (learner.critic, k - 12)
        off = net.offsets[j][1]
        assert torch.equal(net.plain[off:off + p.numel()], p.detach().reshape(-1))
    print("Adam step on the views: at most %.2f of the derived tolerance" % worst)

    actor.eval(), critic.eval()
    policy.refresh()
    boards = np.round(c.x * 15).astype(np.uint8)
    probs, value = policy(torch.from_numpy(boards).to(DEV))
    with torch.no_grad():
        want_p, want_v = (copy.deepcopy(m).cpu().double()(torch.from_numpy(c.x).double()).numpy() for m in (actor, critic))
    ep = np.abs(probs.cpu().numpy() - want_p).max()
    ev = np.abs(value.cpu().numpy() - want_v).max() / np.abs(want_v).max()
    print("DevicePolicy.refresh() after the step: probs %.3g, values %.3g of max|v|" % (ep, ev))
    assert ep <= 2e-5 and ev <= 1e-5            # tests/test_gpu_policy.py's f32 tolerances of that kernel
    assert np.abs(want_p - c.want["probs"]).max() > 1e-3                        # the step changed the policy


def test_gradients_of_the_reference_classes_fixture():
    """The device against the recorded float64 gradients of the reference's own ActorNetwork / CriticNetwork with the trained weights
    of policy.npz, on the fixture's 32 rows. The bound is the case's: 8 x stock float32 autograd's own error on these weights."""
    g, w = load_golden("ppo_update.npz"), load_golden("policy.npz")
    nets32 = golden_modules(w, torch.float32)
    c = R.Case(32, None, nets32=nets32, x=g["states"])
    assert all(np.array_equal(a, g[k]) for a, k in zip(c.args[1:], ("actions", "old_log_probs", "advantages", "returns")))
    learner, _, _ = learner_of(nets32)
    got = Call(learner, c, learner.actor.running, learner.critic.running, None, CANARY)
    want = dict(grads=[g["grad.%02d" % k].astype(np.float64) for k in range(24)], losses=g["losses"].astype(np.float64))
    check_case(c, got, "reference classes' fixture (yardstick %.3g)" % c.yardstick, want)
    check_running(c, split_running(learner.actor.running) + split_running(learner.critic.running),
                  [g["running.%d" % k].astype(np.float64) for k in range(8)], "fixture")
