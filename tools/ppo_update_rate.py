"""DevicePPOLearner (PPOAgent.update, agents/ppo_agent.py:357-416) against stock torch on the same GPU.

    python3 tools/ppo_update_rate.py                      the table
    python3 tools/ppo_update_rate.py --trace N [CALLS]    only CALLS (50) loss_and_grad calls at n = N, for a kernel trace:
        rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/ppo_update_rate.py --trace 256
    python3 tools/ppo_update_rate.py --trace-step [CALLS] only CALLS (50) adam_step calls after one loss_and_grad, for a kernel trace
    python3 tools/ppo_update_rate.py --dropout [PARENT.so] the dropout table: loss_and_grad and update() with p = 0 and p = 0.2 next to
        stock torch's modules with dropout.p 0 and 0.2, and, given another build of the library (e.g. the parent commit's, python -m
        g2048._build -o PARENT.so in its tree), the same p = 0 calls through that build, all alternating in one run

The reference's actor and critic (16-256-128-64-{4|1}, BatchNorm1d after the first two ReLUs, torch's default init) in training
mode with dropout p = 0 on BOTH sides, at n = 256 (the reference's batch) and 4,096 (the limit). Versions, alternating within
every round:
  torch fwd+loss+bwd    both stock modules' forwards, Categorical, the clipped-surrogate / value / entropy loss,
                        zero_grad(set_to_none=False) and backward(): the yardstick;
  device loss_and_grad  the same function, one g2048_ppo_loss_grad call;
  torch update          the whole update(): the no-gradient block (two critic forwards, returns, normalised advantages), then 8
                        epochs of the above with clip_grad_norm_(0.5) per network and two torch.optim.Adam steps;
  device update         the same with learner.advantages and learner.loss_and_grad, the clipping and the SAME stock Adam running on
                        the attached views;
  stock tail            what ends an epoch of "device update": clip_grad_norm_(0.5) per network and two stock Adam steps on the
                        attached views (the gradients are those of one loss_and_grad call);
  device adam_step      the same in two launches, learner.adam_step(losses), the NaN gate included;
  device update()       learner.update(): "device update" with adam_step for the stock tail, on a learner of its own.
The reference's `if torch.isnan(loss): continue` is left out of the stock versions (it is a host synchronisation per epoch);
adam_step decides it on the device.
A round times REPS back-to-back calls of a version between one event pair and divides (the device clock), and takes the host's
perf_counter around the same calls before it waits for the device (the host-enqueue clock); median of 7 rounds after 2 warm-up
rounds, min - max of the device clock in brackets. Before timing, the device gradients and stock torch's float32 ones are both
compared with the modules' float64 autograd on the same GPU, per tensor as max|g - g64| / max|g64|.
Output: one text table (profiles/r23_ppo_update_rate.txt, profiles/r25_ppo_step_rate.txt and profiles/r26_ppo_dropout_rate.txt keep
runs)."""
import copy
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import __graft_entry__ as ge  # noqa: E402

ge.import_package()
from g2048 import DevicePPOLearner, ops  # noqa: E402

dev = torch.device("cuda")
REPS, EPOCHS = 10, 8
GAMMA, CLIP, VALUE_COEF, ENTROPY_COEF, LR, MAX_NORM = 0.995, 0.3, 0.4, 0.05, 5e-4, 0.5


class Net(nn.Module):                   # the reference's structure and forward, stock torch, default init, dropout p = 0
    def __init__(self, n_out):
        super().__init__()
        self.fc1, self.bn1 = nn.Linear(16, 256), nn.BatchNorm1d(256)
        self.fc2, self.bn2 = nn.Linear(256, 128), nn.BatchNorm1d(128)
        self.fc3, self.fc4 = nn.Linear(128, 64), nn.Linear(64, n_out)
        self.dropout, self.softmax = nn.Dropout(0.0), n_out == 4

    def forward(self, x):
        x = torch.relu(self.fc1(x))
        if x.shape[0] > 1:
            x = self.bn1(x)
        x = torch.relu(self.fc2(self.dropout(x)))
        if x.shape[0] > 1:
            x = self.bn2(x)
        x = self.fc4(torch.relu(self.fc3(self.dropout(x))))
        return torch.softmax(x, -1) if self.softmax else x


def event_time(fn):
    """(device seconds, host-enqueue seconds) per call."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / REPS, host / REPS


def alternate(versions, warmup, rounds):
    """{name: [(device seconds, host-enqueue seconds) per call and round]}: every round runs each version, in order."""
    times = {name: [] for name, _ in versions}
    for r in range(warmup + rounds):
        for name, fn in versions:
            dt = event_time(fn)
            if r >= warmup:
                times[name].append(dt)
    return times


def torch_loss(actor, critic, x, actions, old, adv, ret):
    dist = torch.distributions.Categorical(probs=actor(x))
    ratio = torch.exp(dist.log_prob(actions) - old)
    actor_loss = -torch.min(ratio * adv, torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * adv).mean()
    value_loss = nn.functional.mse_loss(critic(x).squeeze(-1), ret)
    return actor_loss + VALUE_COEF * value_loss - ENTROPY_COEF * dist.entropy().mean()


def torch_step(actor, critic, *args):
    loss = torch_loss(actor, critic, *args)
    actor.zero_grad(set_to_none=False)
    critic.zero_grad(set_to_none=False)
    loss.backward()
    return loss


def torch_update(actor, critic, opts, x, nx, actions, old, rewards, dones):
    with torch.no_grad():
        values, next_values = critic(x).squeeze(-1), critic(nx).squeeze(-1)
        ret = rewards + GAMMA * next_values * (1 - dones)
        adv = ret - values
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    for _ in range(EPOCHS):
        torch_step(actor, critic, x, actions, old, adv, ret)
        for net, opt in zip((actor, critic), opts):
            nn.utils.clip_grad_norm_(net.parameters(), MAX_NORM)
            opt.step()


def device_update(learner, actor, critic, opts, x, nx, actions, old, rewards, dones):
    ret, adv = learner.advantages(x, nx, rewards, dones, GAMMA)
    for _ in range(EPOCHS):
        learner.loss_and_grad(x, actions, old, adv, ret)
        for net, opt in zip((actor, critic), opts):
            nn.utils.clip_grad_norm_(net.parameters(), MAX_NORM)
            opt.step()


def stock_tail(actor, critic, opts):
    for net, opt in zip((actor, critic), opts):
        nn.utils.clip_grad_norm_(net.parameters(), MAX_NORM)
        opt.step()


def inputs(actor64, critic64, n):
    x = ops.synth_boards(n, seed=3, device=dev).float() / 15.0          # PPOAgent.normalize_state
    nx = ops.synth_boards(n, seed=4, device=dev).float() / 15.0
    i = torch.arange(n, device=dev)
    actions = (5 * i + 1) % 4
    with torch.no_grad():
        a64, c64 = copy.deepcopy(actor64), copy.deepcopy(critic64)
        lp = torch.log(a64(x.double()).gather(1, actions.unsqueeze(1)).squeeze(1))
        v = c64(x.double()).squeeze(-1)
    old = (lp + ((37 * i + 11) % 101 - 50) / 100.0).float()
    adv = (((13 * i) % 17 - 8) / 4.0 + 2 * x[:, 0]).float()
    ret = (v + 0.5 + x.sum(1) / 8.0 + ((7 * i) % 11 - 5) / 5.0).float()
    rewards, dones = ((3 * i) % 7).float(), (i % 5 == 0).float()
    return x, nx, actions, old, adv, ret, rewards, dones


def fresh(seed=0):
    torch.manual_seed(seed)
    return Net(4).to(dev).train(), Net(1).to(dev).train()


if sys.argv[1:2] == ["--trace"]:
    n, calls = int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 50
    actor, critic = fresh()
    x, nx, actions, old, adv, ret, rewards, dones = inputs(copy.deepcopy(actor).double(), copy.deepcopy(critic).double(), n)
    learner = DevicePPOLearner(actor, critic, CLIP, VALUE_COEF, ENTROPY_COEF)
    for _ in range(calls):
        learner.loss_and_grad(x, actions, old, adv, ret)
    torch.cuda.synchronize()
    print("%d loss_and_grad calls at n = %d" % (calls, n))
    sys.exit(0)

if sys.argv[1:2] == ["--trace-step"]:
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    actor, critic = fresh()
    x, nx, actions, old, adv, ret, rewards, dones = inputs(copy.deepcopy(actor).double(), copy.deepcopy(critic).double(), 256)
    learner = DevicePPOLearner(actor, critic, CLIP, VALUE_COEF, ENTROPY_COEF)
    learner.attach_params()
    losses = learner.loss_and_grad(x, actions, old, adv, ret)
    for _ in range(calls):
        learner.adam_step(losses, lr=LR, max_norm=MAX_NORM)
    torch.cuda.synchronize()
    print("%d adam_step calls; counters %s" % (calls, learner.opt_counters.tolist()))
    sys.exit(0)

def other_build(path):
    """Another build of the C-ABI next to the product's: the entry points it has, bound as g2048._lib binds them."""
    import ctypes
    from g2048 import _lib
    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name, None)           # a parent build lacks what this tree adds
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def through(lib, fn):
    """fn with every C-ABI call of the package going to `lib`: the same Python path, the other build's host code and kernels."""
    from g2048 import _lib

    def run():
        with _lib.MAIN.swapped(lib):
            return fn()
    return run


def report(n, versions, times, against):
    for name, _ in versions:
        tt, hh = [t for t, _ in times[name]], [h for _, h in times[name]]
        med = statistics.median(tt)
        other = against.get(name, versions[0][0])
        base = statistics.median([t for t, _ in times[other]])
        print("%-7d %-26s %10.1f %22s %10.1f %12.4g %9.2fx %s" % (n, name, med * 1e6, "[%.1f - %.1f]" % (min(tt) * 1e6, max(tt) * 1e6),
                                                                 statistics.median(hh) * 1e6, n / med, base / med, other))


if sys.argv[1:2] == ["--dropout"]:
    parent = other_build(sys.argv[2]) if len(sys.argv) > 2 else None
    P = 0.2
    print("# %d calls per event pair; median of 7 rounds after 2 warm-up rounds, the versions alternating; update() is the advantages block "
          "+ %d epochs, adam_step included; torch update: clip_grad_norm_(%.1f) and stock torch.optim.Adam" % (REPS, EPOCHS, MAX_NORM))
    print("%-7s %-26s %10s %22s %10s %12s %10s" % ("rows", "version", "us", "[min - max] us", "host us", "rows/s", "vs"))
    for n in (256, 4096):
        actor, critic = fresh()
        x, nx, actions, old, adv, ret, rewards, dones = inputs(copy.deepcopy(actor).double(), copy.deepcopy(critic).double(), n)

        def learner_with(p):
            le = DevicePPOLearner(copy.deepcopy(actor), copy.deepcopy(critic), CLIP, VALUE_COEF, ENTROPY_COEF, dropout=p)
            le.attach_params()
            return le

        def torch_with(p):
            mods = copy.deepcopy(actor), copy.deepcopy(critic)
            for m in mods:
                m.dropout.p = p
            return mods, [torch.optim.Adam(m.parameters(), lr=LR) for m in mods]
        grad0, grad2, upd0, upd2 = learner_with(0.0), learner_with(P), learner_with(0.0), learner_with(P)
        (t0, o0), (t2, o2), (u0, uo0), (u2, uo2) = torch_with(0.0), torch_with(P), torch_with(0.0), torch_with(P)
        update = lambda le: le.update(x, actions, old, rewards, nx, dones, epochs=EPOCHS, gamma=GAMMA, lr=LR, max_norm=MAX_NORM)      # noqa: E731
        versions, against = [], {}
        if parent is not None:
            grad_p, upd_p = learner_with(0.0), learner_with(0.0)
            mine = [t.clone() for t in (grad0.loss_and_grad(x, actions, old, adv, ret), grad0.actor.grad, grad0.critic.grad)]
            theirs = [through(parent, lambda: grad_p.loss_and_grad(x, actions, old, adv, ret))(), grad_p.actor.grad, grad_p.critic.grad]
            print("# n = %d: p = 0 through this build and through %s: losses and both gradient buffers %s" % (
                n, os.path.basename(sys.argv[2]), "bit for bit the same" if all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                                                                              for a, b in zip(mine, theirs)) else "DIFFER"))
            versions += [("parent loss_and_grad", through(parent, lambda: grad_p.loss_and_grad(x, actions, old, adv, ret)))]
            against.update({"device loss_and_grad p=0": "parent loss_and_grad", "device update() p=0": "parent update()",
                            "parent update()": "parent update()"})
        versions += [("device loss_and_grad p=0", lambda: grad0.loss_and_grad(x, actions, old, adv, ret)),
                     ("device loss_and_grad p=0.2", lambda: grad2.loss_and_grad(x, actions, old, adv, ret)),
                     ("torch fwd+loss+bwd p=0", lambda: torch_step(*t0, x, actions, old, adv, ret)),
                     ("torch fwd+loss+bwd p=0.2", lambda: torch_step(*t2, x, actions, old, adv, ret)),
                     ] + ([("parent update()", through(parent, lambda: update(upd_p)))] if parent is not None else []) + [
                     ("device update() p=0", lambda: update(upd0)), ("device update() p=0.2", lambda: update(upd2)),
                     ("torch update p=0", lambda: torch_update(*u0, uo0, x, nx, actions, old, rewards, dones)),
                     ("torch update p=0.2", lambda: torch_update(*u2, uo2, x, nx, actions, old, rewards, dones))]
        against.update({"device loss_and_grad p=0.2": "device loss_and_grad p=0", "torch fwd+loss+bwd p=0.2": "torch fwd+loss+bwd p=0",
                        "device update() p=0.2": "device update() p=0", "torch update p=0.2": "torch update p=0",
                        "torch fwd+loss+bwd p=0": "device loss_and_grad p=0", "torch update p=0": "device update() p=0"})
        against.setdefault("device loss_and_grad p=0", "device loss_and_grad p=0")
        against.setdefault("device update() p=0", "device update() p=0")
        times = alternate(versions, 2, 7)
        report(n, versions, times, against)
        med = lambda name: statistics.median([t for t, _ in times[name]]) * 1e6      # noqa: E731
        for what, a, b in (("loss_and_grad", "device loss_and_grad p=0.2", "device loss_and_grad p=0"),
                           ("torch fwd+loss+bwd", "torch fwd+loss+bwd p=0.2", "torch fwd+loss+bwd p=0"),
                           ("update()", "device update() p=0.2", "device update() p=0"), ("torch update", "torch update p=0.2", "torch update p=0")):
            print("# n = %d: %s, p = 0.2 over p = 0: %+.1f us (%+.1f %%)" % (n, what, med(a) - med(b), 100 * (med(a) / med(b) - 1)))
        if parent is not None:
            for mine, theirs in (("device loss_and_grad p=0", "parent loss_and_grad"), ("device update() p=0", "parent update()")):
                tt = [t * 1e6 for t, _ in times[theirs]]
                print("# n = %d: %s against %s: %+.1f us; the parent's own rounds span %.1f us" % (n, mine, theirs, med(mine) - med(theirs),
                                                                                                 max(tt) - min(tt)))
        print("# n = %d: dropout_index of the p = 0.2 update() learner %d, its optimiser counters %s" % (n, upd2.dropout_index, upd2.opt_counters.tolist()))
    sys.exit(0)

print("# %d calls per event pair; median of 7 rounds after 2 warm-up rounds, the versions alternating; an update is the advantages "
      "block + %d epochs with clip_grad_norm_(%.1f) and stock torch.optim.Adam" % (REPS, EPOCHS, MAX_NORM))
print("# workspace of the device pass: %s" % ", ".join("n = %d: %.1f MB" % (n, ops.ppo_train_workspace_bytes(n) / 1e6) for n in (256, 4096)))
print("%-7s %-22s %10s %22s %10s %12s %10s" % ("rows", "version", "us", "[min - max] us", "host us", "rows/s", "vs"))
for n in (256, 4096):
    actor, critic = fresh()                                             # stock torch's
    d_actor, d_critic = copy.deepcopy(actor), copy.deepcopy(critic)     # the device learner's
    actor64, critic64 = copy.deepcopy(actor).double(), copy.deepcopy(critic).double()
    x, nx, actions, old, adv, ret, rewards, dones = inputs(actor64, critic64, n)
    learner = DevicePPOLearner(d_actor, d_critic, CLIP, VALUE_COEF, ENTROPY_COEF)
    learner.attach_params()
    learner.attach_grads()
    torch_step(actor64, critic64, x.double(), actions, old.double(), adv.double(), ret.double())
    want = [p.grad.reshape(-1).clone() for net in (actor64, critic64) for p in net.parameters()]
    torch_step(actor, critic, x, actions, old, adv, ret)
    got32 = [p.grad.reshape(-1).double() for net in (actor, critic) for p in net.parameters()]
    learner.loss_and_grad(x, actions, old, adv, ret)
    got = [p.grad.reshape(-1).double() for net in (d_actor, d_critic) for p in net.parameters()]
    ratio = lambda gs: max(((g - z).abs().max() / z.abs().max()).item() for g, z in zip(gs, want))      # noqa: E731
    r_dev, r_torch = ratio(got), ratio(got32)
    print("# n = %d: worst max|g - g64| / max|g64| over the 24 tensors: device %.3g, torch f32 %.3g" % (n, r_dev, r_torch))
    assert r_dev <= 8 * r_torch, "loss_and_grad does not compute torch's gradients"
    opts = [torch.optim.Adam(net.parameters(), lr=LR) for net in (actor, critic)]
    d_opts = [torch.optim.Adam(net.parameters(), lr=LR) for net in (d_actor, d_critic)]
    versions = [("torch fwd+loss+bwd", lambda: torch_step(actor, critic, x, actions, old, adv, ret)),
                ("device loss_and_grad", lambda: learner.loss_and_grad(x, actions, old, adv, ret)),
                ("torch update", lambda: torch_update(actor, critic, opts, x, nx, actions, old, rewards, dones)),
                ("device update", lambda: device_update(learner, d_actor, d_critic, d_opts, x, nx, actions, old, rewards, dones))]
    # the optimiser tail: a second attached learner for the stock tail (its gradients stay those of one call), a third for adam_step,
    # a fourth for update(), so that no version steps another's weights
    def attached():
        mods = copy.deepcopy(actor), copy.deepcopy(critic)
        le = DevicePPOLearner(*mods, CLIP, VALUE_COEF, ENTROPY_COEF)
        le.attach_params()
        le.attach_grads()
        return le, mods
    tail, tail_mods = attached()
    tail.loss_and_grad(x, actions, old, adv, ret)
    tail_opts = [torch.optim.Adam(net.parameters(), lr=LR) for net in tail_mods]
    stepper, _ = attached()
    step_losses = stepper.loss_and_grad(x, actions, old, adv, ret)
    whole, _ = attached()
    versions += [("stock tail", lambda: stock_tail(*tail_mods, tail_opts)),
                 ("device adam_step", lambda: stepper.adam_step(step_losses, lr=LR, max_norm=MAX_NORM)),
                 ("device update()", lambda: whole.update(x, actions, old, rewards, nx, dones, epochs=EPOCHS, gamma=GAMMA, lr=LR, max_norm=MAX_NORM))]
    times = alternate(versions, 2, 7)
    against = {"torch update": "torch update", "device update": "torch update", "device update()": "device update",
               "stock tail": "stock tail", "device adam_step": "stock tail"}
    for name, _ in versions:
        tt, hh = [t for t, _ in times[name]], [h for _, h in times[name]]
        med = statistics.median(tt)
        other = against.get(name, "torch fwd+loss+bwd")
        base = statistics.median([t for t, _ in times[other]])
        print("%-7d %-22s %10.1f %22s %10.1f %12.4g %9.2fx %s" % (n, name, med * 1e6, "[%.1f - %.1f]" % (min(tt) * 1e6, max(tt) * 1e6),
                                                                 statistics.median(hh) * 1e6, n / med, base / med, other))
    print("# n = %d: optimiser counters of the adam_step learner %s, of the update() learner %s"
          % (n, stepper.opt_counters.tolist(), whole.opt_counters.tolist()))
    med = lambda name, k: statistics.median([t[k] for t in times[name]])      # noqa: E731
    assert med("device adam_step", 0) < med("stock tail", 0) and med("device adam_step", 1) < med("stock tail", 1), "adam_step is not faster than the stock tail"
    assert med("device update()", 0) < med("device update", 0), "update() is not faster than the stock-tail update"
