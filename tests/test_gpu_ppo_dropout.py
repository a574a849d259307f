"""The PPO update's dropout on the MI355X (g2048_ppo_forward_train_dropout, g2048_ppo_loss_grad_dropout, g2048_ppo_dropout_mask,
DevicePPOLearner(dropout=...)): the masks bit for bit against their NumPy restatement; p = 0 bit for bit against the entry points
without dropout; loss parts, all 24 gradient tensors, probabilities, values and running statistics against the stock modules' CPU
float64 autograd with the restated masks written out (tests/ppo_dropout_ref.py) at every edge of the touched kernels; the large
sizes on what is continuous in the ReLU inputs; a whole update of three epochs; the checkpoint state; a poisoned row; the example.

Tolerance: tests/ppo_update_ref.py's per case, 8 x the worst gradient tensor of stock CPU float32 autograd (same masks, float scale)
against float64, for the gradients, the loss parts (one tensor), probabilities, values and each running statistic. The inputs'
conditions are asserted on the CPU by tests/test_ppo_dropout_host.py. Every measured multiple is printed; docs/LOG.md R26.1 has
them."""
import ctypes as C
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import ppo_dropout_ref as D
import ppo_update_ref as R
from conftest import REPO
from test_gpu_ppo_step import LOOP_KW, bits, learner_bits, no_sync
from test_gpu_ppo_update import CANARY, DEV, PAD, check_case, check_running, learner_of, padded, split, split_running, to_dev

pytestmark = pytest.mark.gpu

SEED = D.DROPOUT_SEED


# ------------------------------------------------------------------------------------------------------------- masks --
@pytest.mark.parametrize("n", [1, 2, 17, 33, 257, 4096])
def test_masks_equal_the_restatement(n):
    """ops.ppo_dropout_mask against the NumPy restatement bit for bit: both networks, both sites, p = 0.2 and 0.5, a call index
    below and one above 2^32; nothing is written past the mask."""
    from g2048 import ops
    for net in (0, 1):
        for site in (0, 1):
            F = D.WIDTH[site]
            for p in (0.2, 0.5):
                for call in (3, (1 << 32) + 9):
                    buf = torch.full((n * F + PAD,), 7, dtype=torch.uint8, device=DEV)
                    got = ops.ppo_dropout_mask(n, net, site, p, seed=SEED, call_index=call, out=buf[:n * F].view(n, F))
                    torch.cuda.synchronize()
                    assert bool(torch.all(buf[n * F:] == 7)), "written past the mask"
                    want = D.keep_mask(SEED, call, net, site, p, n)
                    assert np.array_equal(got.cpu().numpy().astype(bool), want), (net, site, p, call)
                    assert set(np.unique(got.cpu().numpy()).tolist()) <= {0, 1}


# --------------------------------------------------------------------------------------------------- p = 0 is today's --
def raw_outputs(c, learner, dropout_entry):
    """losses, both gradient buffers, probs, values and the running statistics after them, through the C entry points themselves:
    the ones without dropout, or the *_dropout ones with p = 0 (and a seed and an index that must not matter)."""
    from g2048 import _lib, ops
    L = _lib.lib()
    x, actions, old, adv, ret = to_dev(*c.args)
    n = c.n
    ws = torch.empty(ops.ppo_train_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    ga, gc = torch.zeros_like(learner.actor.grad), torch.zeros_like(learner.critic.grad)
    losses = torch.zeros(4, dtype=torch.float32, device=DEV)
    run = [learner.actor.running.clone(), learner.critic.running.clone()]
    probs, values = torch.zeros((n, 4), dtype=torch.float32, device=DEV), torch.zeros((n, 1), dtype=torch.float32, device=DEV)
    f, d, stream = C.c_float, C.c_double, _lib.stream_ptr(torch.device(DEV))
    head = (x.data_ptr(), actions.data_ptr(), old.data_ptr(), adv.data_ptr(), ret.data_ptr(), learner.actor.plain.data_ptr(),
            learner.critic.plain.data_ptr(), run[0].data_ptr(), run[1].data_ptr(), f(R.CLIP), f(R.VALUE_COEF), f(R.ENTROPY_COEF))
    tail = (n, ga.data_ptr(), gc.data_ptr(), losses.data_ptr(), ws.data_ptr(), stream)
    if dropout_entry:
        assert L.g2048_ppo_loss_grad_dropout(*head, d(0.0), d(0.0), 77, 5, *tail) == 0
        for w, (net, out) in enumerate(((learner.actor, probs), (learner.critic, values))):
            assert L.g2048_ppo_forward_train_dropout(x.data_ptr(), net.plain.data_ptr(), run[w].data_ptr(), net.n_out, w, d(0.0), 77, 6,
                                                     out.data_ptr(), n, ws.data_ptr(), stream) == 0
    else:
        assert L.g2048_ppo_loss_grad(*head, *tail) == 0
        for w, (net, out) in enumerate(((learner.actor, probs), (learner.critic, values))):
            assert L.g2048_ppo_forward_train(x.data_ptr(), net.plain.data_ptr(), run[w].data_ptr(), net.n_out, out.data_ptr(), n, ws.data_ptr(),
                                             stream) == 0
    torch.cuda.synchronize()
    return [losses, ga, gc, probs, values] + run


@pytest.mark.parametrize("n", [1, 17, 257])
def test_p_zero_is_the_pass_without_dropout(n):
    """DevicePPOLearner(dropout=0.0), ops with dropout=0 and the *_dropout entry points called with p = 0 give the bits of
    g2048_ppo_loss_grad / g2048_ppo_forward_train: losses, all 24 gradient tensors, probabilities, values, running statistics."""
    from g2048 import ops
    c = R.case(n)
    x, actions, old, adv, ret = to_dev(*c.args)
    base, _, _ = learner_of(c.nets32)
    want = raw_outputs(c, base, False)
    names = ("losses", "actor gradients", "critic gradients", "probs", "values", "actor running", "critic running")

    def same(got, what):
        for name, a, b in zip(names, got, want):
            assert torch.equal(bits(a), bits(b)), "%s: %s differ (n = %d)" % (what, name, n)
    same(raw_outputs(c, base, True), "the *_dropout entry points at p = 0")

    learner, _, _ = learner_of(c.nets32, dropout=0.0, dropout_seed=123)
    losses = learner.loss_and_grad(x, actions, old, adv, ret).clone()
    probs, values = learner.probs(x).clone(), learner.values(x).clone()
    same([losses, learner.actor.grad, learner.critic.grad, probs, values, learner.actor.running, learner.critic.running], "the learner")
    assert learner.dropout == (0.0, 0.0) and learner.dropout_index == 3

    run = [base.actor.running.clone(), base.critic.running.clone()]
    losses, ga, gc = ops.ppo_loss_grad(x, actions, old, adv, ret, base.actor.plain, base.critic.plain, run[0], run[1], R.CLIP, R.VALUE_COEF,
                                       R.ENTROPY_COEF, dropout=0.0, seed=9, call_index=4)
    probs = ops.ppo_forward_train(x, base.actor.plain, 4, running=run[0], dropout=0.0, seed=9, call_index=5, net=0)
    values = ops.ppo_forward_train(x, base.critic.plain, 1, running=run[1], dropout=0.0, seed=9, call_index=5, net=1)
    same([losses, ga, gc, probs, values] + run, "ops with dropout = 0")


# ----------------------------------------------------------------------------------- against float64 with the masks --
class DropCall:
    """One ops.ppo_loss_grad call with dropout into padded outputs, on states that have rows to spare; what check_case reads."""

    def __init__(self, learner, c, run_a, run_c, fill=CANARY, index=None, args=None, p=None):
        from g2048 import ops
        x, actions, old, adv, ret = c.args if args is None else args
        n = len(x)
        self.x_all = torch.full((n + 5, 16), float("nan"), dtype=torch.float32, device=DEV)
        self.x_all[:n] = torch.from_numpy(x)
        self.x_kept = self.x_all.clone()
        self.ga_all, ga = padded(ops.ppo_plain_floats(4), fill)
        self.gc_all, gc = padded(ops.ppo_plain_floats(1), fill)
        self.l_all, losses = padded(4, fill)
        nb = ops.ppo_train_workspace_bytes(n)
        self.ws_all = torch.full((nb // 4 + PAD,), float("nan"), dtype=torch.float32, device=DEV)
        self.ws_all[nb // 4:] = fill
        ops.ppo_loss_grad(self.x_all[:n], *to_dev(actions, old, adv, ret), learner.actor.plain, learner.critic.plain, run_a, run_c, *c.coefs,
                          grad_actor=ga, grad_critic=gc, losses=losses, workspace=self.ws_all.view(torch.uint8)[:nb],
                          dropout=c.p if p is None else p, seed=SEED, call_index=c.index if index is None else index)
        torch.cuda.synchronize()
        self.fill = fill
        self.bits = [bits(t) for t in (ga, gc, losses)]
        self.grads = split(learner.actor, ga) + split(learner.critic, gc)
        self.losses = losses.cpu().numpy().astype(np.float64)

    def canaries_intact(self):
        return all(bool(torch.all(t[-PAD:] == self.fill)) for t in (self.ga_all, self.gc_all, self.l_all, self.ws_all)) and \
            torch.equal(bits(self.x_all), bits(self.x_kept))


def forwards(learner, c, run_a, run_c, what):
    """forward_train with dropout, one network at a time, into outputs with rows to spare: (probs, values) as float64; the bound on
    both, the canaries, and the running statistics moved as loss_grad moves them (the buffers given are moved)."""
    from g2048 import ops
    x = to_dev(c.x)[0]
    out = []
    for w, (net, key, running) in enumerate(((learner.actor, "probs", run_a), (learner.critic, "values", run_c))):
        out_all = torch.full((c.n + 9, net.n_out), CANARY, dtype=torch.float32, device=DEV)
        ops.ppo_forward_train(x, net.plain, net.n_out, running=running, out=out_all[:c.n], dropout=D.pair(c.p)[w], seed=SEED,
                              call_index=c.index, net=w)
        torch.cuda.synchronize()
        assert bool(torch.all(out_all[c.n:] == CANARY)), "%s: rows past n were written" % what
        got = out_all[:c.n].cpu().numpy().astype(np.float64).reshape(c.want[key].shape)
        e = R.rel(got, c.want[key])
        print("%s: forward_train %s %.3g of max = %.2f x the yardstick" % (what, key, e, e / c.yardstick))
        assert e <= c.bound, what
        out.append(out_all[:c.n].clone())
    return out


CASES = [(n, D.P) for n in D.GRAD_SIZES] + [(17, p) for p in D.EXTRA_P]


@pytest.mark.parametrize("key", CASES, ids=str)
def test_loss_grad_and_forwards_against_float64_with_the_masks(key):
    """Per case: the four loss parts, all 24 gradient tensors, forward_train's probabilities and values and the running statistics
    against CPU float64 with the restated masks; canaries after every output, after the workspace and in the rows past n of the
    states; a second call gives the same bits. n = 1: the BatchNorm gradients are exactly 0 and the running statistics keep their
    bits. p = 1e-12 (T = 0, every element kept, the float scale exactly 1) also gives the bits of the pass without dropout."""
    from g2048 import ops
    n, p = key
    c = D.case(n, p)
    what = "n = %d, p = %r" % (n, p)
    learner, _, _ = learner_of(c.nets32)
    run0 = (learner.actor.running.clone(), learner.critic.running.clone())
    run_a, run_c = run0[0].clone(), run0[1].clone()
    got = DropCall(learner, c, run_a, run_c)
    assert got.canaries_intact(), "%s: written past the end of an output, or into the states" % what
    check_case(c, got, what)
    if n == 1:
        assert torch.equal(run_a, run0[0]) and torch.equal(run_c, run0[1]), "n = 1 moved the running statistics"
        assert all(not got.grads[k].any() for k in (2, 3, 6, 7, 14, 15, 18, 19)), "n = 1: a BatchNorm gradient is not exactly 0"
    else:
        check_running(c, split_running(run_a) + split_running(run_c), c.want["running"], what)
    again = DropCall(learner, c, None, None, fill=-3.0)
    assert again.canaries_intact() and all(torch.equal(a, b) for a, b in zip(got.bits, again.bits)), "%s: a second call differs" % what
    fa, fc = run0[0].clone(), run0[1].clone()
    forwards(learner, c, fa, fc, what)
    assert torch.equal(fa, run_a) and torch.equal(fc, run_c), "forward_train and loss_grad move the running statistics differently"
    if p == 1e-12:
        x, actions, old, adv, ret = to_dev(*c.args)
        plain = ops.ppo_loss_grad(x, actions, old, adv, ret, learner.actor.plain, learner.critic.plain)
        assert all(torch.equal(bits(a), b) for a, b in zip((plain[1], plain[2], plain[0]), got.bits)), "T = 0 is not the pass without dropout"


@pytest.mark.parametrize("n", D.LARGE_SIZES)
def test_large_batches_on_what_is_continuous(n):
    """n = 1,025 and 4,096 at p = 0.2. Every row is distinct after the first dropout site, and some of the n x 448 ReLU inputs per
    network lie within RELU_MARGIN of zero (ppo_dropout_ref.LARGE_NEAR_ZERO, counted on the CPU), where one float32 rounding flips a
    ReLU's gradient: the gradients are not compared here (backward parity at 257 rows and the masks at 4,096 cover the backward's
    indexing). What is continuous in the ReLU inputs is: probabilities and values per row, the four loss parts, the running
    statistics, each against float64 within 8 x the yardstick, here the float32 masked modules' own worst error on those same
    quantities (at least 8 float32 roundings, 8 x 2^-24, the floor of the advantages block's test). Two calls with one index give
    the same bits in every output and gradient; another index gives other gradients."""
    c = D.large_case(n)
    what = "n = %d" % n
    learner, _, _ = learner_of(c.nets32)
    run_a, run_c = learner.actor.running.clone(), learner.critic.running.clone()
    got = DropCall(learner, c, run_a, run_c)
    assert got.canaries_intact()
    e_loss = R.rel(got.losses, c.want["losses"])
    print("%s: loss parts %.3g = %.2f x the yardstick %.3g" % (what, e_loss, e_loss / c.yardstick, c.yardstick))
    assert np.isfinite(got.losses).all() and e_loss <= c.bound
    check_running(c, split_running(run_a) + split_running(run_c), c.want["running"], what)
    forwards(learner, c, learner.actor.running.clone(), learner.critic.running.clone(), what)
    again = DropCall(learner, c, None, None, fill=-3.0)
    assert all(torch.equal(a, b) for a, b in zip(got.bits, again.bits)), "two calls with one index differ"
    other = DropCall(learner, c, None, None, index=c.index + 1)
    assert not torch.equal(other.bits[0], got.bits[0]) and not torch.equal(other.bits[1], got.bits[1]), "another index, the same gradients"
    assert all(np.isfinite(g).all() for g in got.grads)


# -------------------------------------------------------------------------------------------------- a whole update --
def device_loop(c, **kw):
    """tests/test_gpu_ppo_step.py's device_loop on a learner with dropout."""
    learner, actor, critic = learner_of(c.nets32, **kw)
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
        norms = learner.adam_step(losses, **LOOP_KW)
        ep["norm_bits"] = bits(norms).clone()
        ep["delta"] = [p.detach().cpu().numpy().astype(np.float64).reshape(-1) - s for p, s in zip(params, start)]
        out["epochs"].append(ep)
    torch.cuda.synchronize()
    out["bits"] = learner_bits(learner)
    out["running"] = split_running(learner.actor.running) + split_running(learner.critic.running)
    out["tracked"] = [int(bn.num_batches_tracked) for m in (actor, critic) for bn in (m.bn1, m.bn2)]
    out["counters"], out["index"] = learner.opt_counters.tolist(), learner.dropout_index
    return out


def test_whole_update_three_epochs_with_dropout():
    """The closed-loop case of tests/test_gpu_ppo_step.py (n = 48, 3 epochs) with p = 0.2 against stock_loop_masked, call indices 0, 1
    for the advantages block and 2, 3, 4 for the epochs, under that test's bounds: returns and advantages within advantage_bound, per
    epoch the loss parts within the case's bound and each tensor's accumulated change off from float64's by at most 8 x the float32
    run's deviation (never tighter than 2^-23 max|p|), running statistics within the bound. Then update(epochs=3) from the same
    start with torch's synchronisation check set to raise: dropout_index 5 and the manual sequence's bits."""
    c = D.loop_case()
    kw = dict(dropout=D.P, dropout_seed=SEED)
    got = device_loop(c, **kw)
    e_adv = max(R.rel(got["returns"], c.want["adv"]["returns"]), R.rel(got["advantages"], c.want["adv"]["advantages"]))
    print("returns and advantages %.3g of their maxima (bound %.3g)" % (e_adv, c.adv_bound))
    assert e_adv <= c.adv_bound
    for e, (g, w, f) in enumerate(zip(got["epochs"], c.want["epochs"], c.f32["epochs"])):
        e_loss = R.rel(g["losses"], w["losses"])
        worst, where = 0.0, -1
        for k, (dg, dw, df, s) in enumerate(zip(g["delta"], w["delta"], f["delta"], c.want["start"])):
            err, mirror = np.abs(dg - dw).max(), np.abs(df - dw).max()
            tol = max(R.F32_FACTOR * mirror, 2.0 ** -23 * np.abs(s).max())
            if err / tol > worst:
                worst, where = err / tol, k
        print("epoch %d: loss parts %.2f x the yardstick %.3g; parameter changes at most %.2f of their bound (tensor %d)"
              % (e, e_loss / c.yardstick, c.yardstick, worst, where))
        assert np.isfinite(g["losses"]).all() and e_loss <= c.bound
        assert worst <= 1.0, "epoch %d, tensor %d: p_e - p_0 is off by %.2f of its bound" % (e, where, worst)
    check_running(c, got["running"], c.want["running"], "after %d epochs" % R.LOOP_EPOCHS)
    assert got["tracked"] == [3, 3, 5, 5] == c.want["tracked"]
    assert got["counters"] == [3, 3, 0, 0] and got["index"] == 5

    learner, actor, critic = learner_of(c.nets32, **kw)
    learner.attach_params()
    x, nx, rewards, dones = to_dev(*c.inputs)
    actions, old = to_dev(c.actions, c.old)
    with no_sync():
        losses, norms = learner.update(x, actions, old, rewards, nx, dones, epochs=R.LOOP_EPOCHS, **LOOP_KW)
    torch.cuda.synchronize()
    assert learner.dropout_index == 5 and learner.dropout_state() == (SEED, 5)
    assert all(torch.equal(a, b) for a, b in zip(got["bits"], learner_bits(learner))), "update() and the manual sequence leave other bits"
    for e, ep in enumerate(got["epochs"]):
        assert torch.equal(bits(losses[e]), ep["loss_bits"]) and torch.equal(bits(norms[e]), ep["norm_bits"]), "epoch %d" % e


def test_dropout_state_round_trip():
    """set_dropout_state(dropout_state()) on a fresh learner with the same weights reproduces the next loss_and_grad bit for bit;
    without it (index 0, another seed) the gradients differ."""
    c = D.case(17)
    args = to_dev(*c.args)
    first, _, _ = learner_of(c.nets32, dropout=D.P, dropout_seed=SEED)
    first.probs(args[0])
    first.advantages(args[0], args[0], args[3], args[3])
    state = first.dropout_state()
    assert state == (SEED, 3)
    losses = first.loss_and_grad(*args)
    want = [bits(t) for t in (losses, first.actor.grad, first.critic.grad)]
    assert first.dropout_state() == (SEED, 4)
    fresh, _, _ = learner_of(c.nets32, dropout=D.P, dropout_seed=SEED + 1)
    losses = fresh.loss_and_grad(*args)
    assert not torch.equal(bits(fresh.actor.grad), want[1])
    fresh.set_dropout_state(state)
    losses = fresh.loss_and_grad(*args)
    assert all(torch.equal(bits(t), w) for t, w in zip((losses, fresh.actor.grad, fresh.critic.grad), want))
    with pytest.raises(ValueError, match="negative"):
        fresh.set_dropout_state((SEED, -1))


@pytest.mark.parametrize("n", [1, 17])
def test_poisoned_row_shows_as_in_stock_float32_with_the_masks(n):
    """The last row's state is +inf, p = 0.2: dropout is a multiplication, so a dropped infinity becomes NaN as in torch. Each loss
    part is finite, NaN, +inf or -inf as stock CPU float32's is on the masked modules (Categorical evaluated by hand, which in float32
    is torch's bit for bit and does not refuse NaN probabilities), and each of the 24 gradient tensors holds a non-finite value
    exactly when stock's does."""
    c = D.case(n)
    x = c.x.copy()
    x[-1] = np.inf
    args = (x,) + c.args[1:]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f32 = R.stock_update(c.masked32, *args, eps=R.F32_EPS)
    learner, _, _ = learner_of(c.nets32)
    got = DropCall(learner, c, None, None, args=args)
    assert got.canaries_intact()
    print("n = %d, inf state: loss parts %s (stock float32 %s); non-finite gradient tensors %d of 24 (stock %d)"
          % (n, R.classes(got.losses), R.classes(f32["losses"]), sum(R.nonfinite(got.grads)), sum(R.nonfinite(f32["grads"]))))
    assert R.classes(got.losses) == R.classes(f32["losses"])
    assert R.nonfinite(got.grads) == R.nonfinite(f32["grads"])


def test_example_runs_with_dropout():
    """examples/ppo_rollout.py --learner device --optimizer device --dropout 0.2 runs to the end: a finite loss, eight Adam steps on
    each network, ten training-mode forwards counted."""
    script = os.path.join(REPO, "examples", "ppo_rollout.py")
    out = subprocess.run([sys.executable, script, "--envs", "1024", "--steps", "16", "--learner", "device", "--optimizer", "device",
                          "--dropout", "0.2"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = re.search(r"device update on 256 sampled transitions \(of 16384\): loss (\S+) \(actor (\S+), value (\S+), entropy (\S+)\) after 8 epochs",
                     out.stdout)
    assert line and all(np.isfinite(float(v)) for v in line.groups()), out.stdout[-2000:]
    counts = re.search(r"device optimizer: (\d+) / (\d+) Adam steps applied", out.stdout)
    assert counts and [int(v) for v in counts.groups()] == [8, 8], out.stdout[-2000:]
    assert "dropout p = 0.2: 10 training-mode forwards drew masks" in out.stdout, out.stdout[-2000:]
