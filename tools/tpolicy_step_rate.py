"""DeviceTransformerPolicy.adam_step and update (the NaN gate, clipping and Adam of a PPO epoch on the device,
g2048_tpolicy_adam_step) against the path they replace, on the same GPU in the same run.

    python3 tools/tpolicy_step_rate.py [--out profiles/r30_tpolicy_step_rate.txt]

The reference's shape (dim_ff 2,048, 2 layers, 702,217 floats; torch's default init, the heads x 8). Two networks from the same
weights, both with attach_params():
  stock   attach_grads(), torch.nn.utils.clip_grad_norm_(0.5), a stock torch.optim.Adam.step() on the attached views and
          net.refresh() (which then only packs): what examples/tpolicy_update.py did before adam_step existed;
  device  net.adam_step(losses): three launches and the same pack.
Timed, alternating within every round:
  the tail of an epoch    stock tail | device adam_step | the step's three launches without the pack | the pack launch alone;
  a whole update          advantages + 8 x (loss_and_grad + stock tail) | net.update(epochs=8), at N = 256 and N = 1,024 boards.
A round times REPS back-to-back calls of a version between one event pair (the device clock) and inside a host clock that ends
in a synchronise, and divides; the host's time to enqueue the calls is the third figure. Median of 7 rounds after 2 warm-up rounds,
min - max in brackets. Before timing, one epoch and one update(epochs=8) of each path from the same weights are compared: faster and different
is not faster. Output: one text table, printed and written to --out."""
import argparse
import copy
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import __graft_entry__ as ge  # noqa: E402

ge.import_package()
from g2048 import DeviceTransformerPolicy, ops  # noqa: E402

dev = torch.device("cuda")
DIM_FF, LAYERS, EPOCHS = 2048, 2, 8
LR, MAX_NORM = 3e-4, 0.5
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


class TPolicy(nn.Module):               # the reference's structure and forward, stock torch, default init
    def __init__(self, dim_ff, layers=LAYERS):
        super().__init__()
        self.embedding = nn.Linear(1, 64)
        layer = nn.TransformerEncoderLayer(d_model=64, nhead=4, dim_feedforward=dim_ff, batch_first=True)
        self.transformer_encoder = nn.TransformerEncoder(layer, num_layers=layers, enable_nested_tensor=False)
        self.fc1, self.fc2 = nn.Linear(1024, 128), nn.Linear(128, 64)
        self.actor, self.critic = nn.Linear(64, 4), nn.Linear(64, 1)

    def forward(self, x):
        n = x.size(0)
        x = self.transformer_encoder(self.embedding(x.view(n, 16, 1))).reshape(n, -1)
        x = torch.relu(self.fc2(torch.relu(self.fc1(x))))
        return torch.softmax(self.actor(x), dim=-1), self.critic(x)


def timed(fn, reps):
    """(device seconds, host seconds to the synchronise, host seconds to enqueue) per call."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return e0.elapsed_time(e1) * 1e-3 / reps, (t2 - t0) / reps, (t1 - t0) / reps


def alternate(versions, reps, warmup=2, rounds=7):
    times = {name: [] for name, _ in versions}
    for r in range(warmup + rounds):
        for name, fn in versions:
            dt = timed(fn, reps)
            if r >= warmup:
                times[name].append(dt)
    return times


def cell(rows, k):
    v = [r[k] * 1e6 for r in rows]
    return "%9.1f us [%8.1f - %8.1f]" % (statistics.median(v), min(v), max(v))


def report(title, times, base):
    say(title)
    say("  %-44s %-33s %-33s %s" % ("version", "device clock", "host clock to the synchronise", "host enqueue"))
    for name, rows in times.items():
        say("  %-44s %-33s %-33s %s" % (name, cell(rows, 0), cell(rows, 1), cell(rows, 2)))
    med = lambda name, k: statistics.median(r[k] for r in times[name])      # noqa: E731
    for name in times:
        if name != base:
            say("  %s / %s: %.2f x on the device clock, %.2f x on the host clock"
                % (base, name, med(base, 0) / med(name, 0), med(base, 1) / med(name, 1)))


def inputs(n):
    boards, nxt = ops.synth_boards(n, seed=29 + n, device=dev), ops.synth_boards(n, seed=1029 + n, device=dev)
    i = torch.arange(n, device=dev)
    gen = torch.Generator(device=dev).manual_seed(n)
    actions = (5 * i + 1) % 4
    old = (-1.4 + 0.5 * torch.randn(n, generator=gen, device=dev)).float()
    rewards = (((13 * i) % 17) / 4.0).float()
    dones = ((i % 11) == 0).float()
    return boards, actions, old, rewards, nxt, dones


class Stock:
    """The path adam_step replaces: the module's parameters and gradients as views, stock clipping and Adam, refresh()."""

    def __init__(self, model):
        self.net = DeviceTransformerPolicy(copy.deepcopy(model))
        self.net.attach_params()
        self.net.attach_grads()
        self.params = list(self.net.model.parameters())
        self.opt = torch.optim.Adam(self.params, lr=LR)

    def tail(self):
        torch.nn.utils.clip_grad_norm_(self.params, max_norm=MAX_NORM)
        self.opt.step()
        self.net.refresh()

    def update(self, boards, actions, old, rewards, nxt, dones):
        net = self.net
        returns, adv = net.advantages(boards, nxt, rewards, dones)
        for _ in range(EPOCHS):
            net.loss_and_grad(boards, actions, old, adv, returns)
            self.tail()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r30_tpolicy_step_rate.txt"))
    a = ap.parse_args()
    say("device: %s; torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    torch.manual_seed(29)
    model = TPolicy(DIM_FF).to(dev).eval()
    with torch.no_grad():
        model.actor.weight.mul_(8.0)
        model.critic.weight.mul_(8.0)
    stock = Stock(model)
    net = DeviceTransformerPolicy(copy.deepcopy(model))
    net.attach_params()
    say("dim_ff %d, %d layers: %d floats in each of plain, grad, exp_avg, exp_avg_sq; step workspace %d bytes"
        % (DIM_FF, LAYERS, net.plain.numel(), ops.tpolicy_step_workspace_bytes(DIM_FF, LAYERS)))

    # faster and different is not faster: one epoch, then one whole update, of each path from the same weights
    args = inputs(256)
    one_s, one_d = Stock(model), DeviceTransformerPolicy(copy.deepcopy(model))
    for n_ in (one_s.net, one_d):
        returns, adv = n_.advantages(args[0], args[4], args[3], args[5])
        first_losses, _, _ = n_.loss_and_grad(args[0], args[1], args[2], adv, returns)
    one_s.tail()
    one_d.adam_step(first_losses, lr=LR, max_norm=MAX_NORM)
    torch.cuda.synchronize()
    say("after ONE epoch at N = 256 from the same weights: max|device - stock| / max|w| = %.3g in the weights (the step moved them by %.3g)"
        % (float((one_d.plain.double() - one_s.net.plain.double()).abs().max() / one_d.plain.abs().max()),
           float((one_d.plain.double() - model_plain(model)).abs().max() / one_d.plain.abs().max())))
    del one_s, one_d
    stock.update(*args)
    losses, norms = net.update(*args, epochs=EPOCHS, lr=LR, max_norm=MAX_NORM)
    torch.cuda.synchronize()
    w_dev, w_stock = net.plain.double(), stock.net.plain.double()
    say("after update(epochs=%d) at N = 256 from the same weights: max|device - stock| / max|w| = %.3g in the weights (the step moved "
        "them by %.3g); counters %s; norms %.4g .. %.4g"
        % (EPOCHS, float((w_dev - w_stock).abs().max() / w_stock.abs().max()),
           float((w_dev - model_plain(model)).abs().max() / w_stock.abs().max()),
           net.opt_counters.tolist(), float(norms.min()), float(norms.max())))

    # the tail of an epoch, on the gradient of one loss_and_grad at N = 256 in each network
    boards, actions, old, rewards, nxt, dones = args
    for n_ in (stock.net, net):
        returns, adv = n_.advantages(boards, nxt, rewards, dones)
        step_losses, _, _ = n_.loss_and_grad(boards, actions, old, adv, returns)
    norm = torch.empty((), dtype=torch.float32, device=dev)
    workspace = torch.empty(ops.tpolicy_step_workspace_bytes(DIM_FF, LAYERS), dtype=torch.uint8, device=dev)
    versions = [("stock: clip_grad_norm_ + Adam.step + refresh", stock.tail),
                ("device: adam_step (3 launches + pack)", lambda: net.adam_step(step_losses, lr=LR, max_norm=MAX_NORM)),
                ("device: the 3 launches alone", lambda: ops.tpolicy_adam_step(
                    net.plain, net.grad, net.exp_avg, net.exp_avg_sq, net.dim_ff, net.n_layers, net.opt_counters, losses=step_losses, lr=LR,
                    max_norm=MAX_NORM, norm=norm, workspace=workspace)),
                ("the pack launch alone", lambda: net.pack(net.plain, net.dim_ff, net.n_layers, net.precision, out=net.packed))]
    report("the tail of an epoch (REPS 20)", alternate(versions, 20), versions[0][0])

    for n in (256, 1024):
        args = inputs(n)
        versions = [("stock: advantages + %d x (loss_and_grad + tail)" % EPOCHS, lambda: stock.update(*args)),
                    ("device: update(epochs=%d)" % EPOCHS, lambda: net.update(*args, epochs=EPOCHS, lr=LR, max_norm=MAX_NORM))]
        report("a whole update at N = %d (REPS 3)" % n, alternate(versions, 3), versions[0][0])
    say("counters at the end: %s (applied, skipped for a NaN loss, skipped for a norm that is not finite)" % net.opt_counters.tolist())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


def model_plain(model):
    from g2048 import tpolicy
    return tpolicy.flatten(tpolicy.parse(model)).double()


if __name__ == "__main__":
    main()
