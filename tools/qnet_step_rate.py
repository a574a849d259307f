"""DeviceQNetwork.adamw_step (gradient clipping and AdamW of DQNAgent.train_step, agents/hybrid.py:1057-1059, on the device) against
the stock torch tail it replaces, on the same GPU.

    python3 tools/qnet_step_rate.py                       the table
    python3 tools/qnet_step_rate.py --trace [CALLS]       only CALLS (50) adamw_step calls, for a kernel trace:
        rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/qnet_step_rate.py --trace
        python3 tools/qnet_step_rate.py --phases OUT      that trace as one line per kernel

The reference's shape (dim_ff 2048, 2 layers, torch's default init: 1,326,184 floats with the four LayerNorm-eps slots). Both sides start from the gradient of one
loss_and_grad call at n = 256, which is not timed and not repeated (clipping leaves the gradient clipped, so from the second call on
neither side clips any further). Versions, alternating within every round:
  torch tail            clip_grad_norm_(max_norm 10) + AdamW.step() + CosineAnnealingLR.step() + net.refresh() on a network whose
                        .grad fields are views into net.grad (attach_grads): what examples/dqn_replay.py --train runs without
                        --device-step;
  device adamw_step     net.adamw_step(g2048.cosine_lr(t)) on a network with attach_params(): the norm, the update and the pack;
  device, not attached  the same on a network without attach_params(): adamw_step also loads the module from net.plain.
Two clocks. Device time: REPS back-to-back calls between one event pair, divided. Host enqueue time: perf_counter around the same
REPS calls WITHOUT a synchronise (the queue is drained before the clock starts and after it stops), divided: what the Python
thread pays before it can go on. Median of 7 rounds after 2 warm-up rounds, min - max in brackets.
Before timing, one update of each side from the same weights and gradient is compared with qnet.adamw_step_reference in float64.
Output: one text table (profiles/r20_qnet_step_rate.txt keeps a run)."""
import copy
import csv
import glob
import os
import statistics
import sys
import time
from collections import defaultdict

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

def phases(directory):
    """One line per kernel of a rocprofv3 --kernel-trace csv: launches, median and minimum duration (qs_norm and qs_update are the
    update's two; the pack is qnet_pack_params_kernel and pack_matrix_kernel; the rest is the set-up)."""
    for f in sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)):
        by = defaultdict(list)
        for row in csv.DictReader(open(f)):
            by[row.get("Kernel_Name", "")].append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
        calls = max([len(v) for name, v in by.items() if "qs_norm_kernel" in name] or [1])
        total = 0.0
        for name, v in sorted(by.items()):
            v.sort()
            med = v[len(v) // 2] * 1e-3
            total += med * len(v)
            print("%-90s launches %5d   %8.1f us [%8.1f]" % (name[:90], len(v), med, v[0] * 1e-3))
        print("sum of the kernel medians over a call's launches (%d calls traced): %.1f us a call" % (calls, total / calls))


if sys.argv[1:2] == ["--phases"]:
    phases(sys.argv[2])
    sys.exit(0)

import __graft_entry__ as ge  # noqa: E402

g2048 = ge.import_package()
from g2048 import DeviceQNetwork, ops, qnet  # noqa: E402

dev = torch.device("cuda")
DIM_FF, LAYERS, REPS, N, MAX_NORM = 2048, 2, 10, 256, 10.0


class QNet(nn.Module):                  # the reference's structure and forward, stock torch, default init
    def __init__(self, dim_ff=DIM_FF, layers=LAYERS):
        super().__init__()
        self.cnn = nn.Sequential(nn.Conv2d(1, 32, kernel_size=2, stride=1, padding=1), nn.ReLU(),
                                 nn.Conv2d(32, 64, kernel_size=2, stride=1, padding=0), nn.ReLU())
        self.embedding = nn.Linear(1024, 128)
        self.transformer = nn.TransformerEncoder(nn.TransformerEncoderLayer(d_model=128, nhead=8, dim_feedforward=dim_ff), layers,
                                                 enable_nested_tensor=False)
        self.fc = nn.Linear(128, 4)

    def forward(self, x):               # one sequence of B tokens
        h = self.embedding(self.cnn(x.view(-1, 1, 4, 4)).view(x.shape[0], -1))
        return self.fc(self.transformer(h.unsqueeze(1)).squeeze(1))


def both_clocks(fn):
    """(device seconds, host enqueue seconds) per call over REPS back-to-back calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    for _ in range(REPS):
        fn()
    t1 = time.perf_counter()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / REPS, (t1 - t0) / REPS


def alternate(versions, warmup, rounds):
    times = {name: ([], []) for name, _ in versions}
    for r in range(warmup + rounds):
        for name, fn in versions:
            d, h = both_clocks(fn)
            if r >= warmup:
                times[name][0].append(d)
                times[name][1].append(h)
    return times


torch.manual_seed(0)
model = QNet().to(dev).eval()
stock, attached, loose = (DeviceQNetwork(copy.deepcopy(model)) for _ in range(3))
boards = ops.synth_boards(N, seed=3, device=dev)
i = torch.arange(N, device=dev)
actions, targets, weights = (5 * i + 1) % 4, (((37 * i + 11) % 101 - 50) / 25.0).to(torch.float32), (0.25 + ((13 * i) % 16) / 16.0).to(torch.float32)
for net in (stock, attached, loose):
    net.loss_and_grad(boards, actions, targets, weights)
gradient = stock.grad.clone()
stock.attach_grads()
attached.attach_params()
params = list(stock.model.parameters())
optimizer = torch.optim.AdamW(params, lr=1e-3, weight_decay=1e-4)
scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=150000, eta_min=1e-4)
clock = {"t": 0}


def torch_tail():
    torch.nn.utils.clip_grad_norm_(params, max_norm=MAX_NORM)
    optimizer.step()
    scheduler.step()
    stock.refresh()


def device_tail(net):
    def fn():
        net.adamw_step(g2048.cosine_lr(clock["t"]), max_norm=MAX_NORM)
        clock["t"] += 1
    return fn


if sys.argv[1:2] == ["--trace"]:
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    fn = device_tail(attached)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    print("%d adamw_step calls at dim_ff %d, %d layers" % (calls, DIM_FF, LAYERS))
    sys.exit(0)

# ---- one update of each side from the same state, against the float64 yardstick
eps_at, o = [], 0
for t in stock.parsed.plain_tensors():
    if isinstance(t, torch.Tensor):
        o += t.numel()
    else:
        eps_at.append(o)
        o += 1
before = stock.plain.clone()
want = qnet.adamw_step_reference(before, gradient, torch.zeros_like(before), torch.zeros_like(before), eps_at, g2048.cosine_lr(0), 1,
                                 max_norm=MAX_NORM)[0]
torch_tail()
device_tail(attached)()
device_tail(loose)()
dev_of = lambda x: ((x.double() - want).abs().max() / want.abs().max()).item()
print("# dim_ff %d, %d layers, %d floats; %d calls per clock pair; median of 7 rounds after 2 warm-up rounds, the versions alternating"
      % (DIM_FF, LAYERS, before.numel(), REPS))
print("# first update against the float64 yardstick, max|w - w64| / max|w64|: torch tail %.3g, device %.3g, device not attached %.3g; gradient "
      "norm %.4g" % (dev_of(stock.plain), dev_of(attached.plain), dev_of(loose.plain), float(gradient.double().norm())))
assert dev_of(attached.plain) <= 8 * max(dev_of(stock.plain), 1e-8), "adamw_step does not compute torch's update"

versions = [("torch tail", torch_tail), ("device adamw_step", device_tail(attached)), ("device, not attached", device_tail(loose))]
times = alternate(versions, 2, 7)
print("%-22s %12s %22s %10s %14s %22s %10s" % ("version", "device us", "[min - max] us", "vs torch", "host enqueue us", "[min - max] us", "vs torch"))
base = [statistics.median(x) for x in times["torch tail"]]
for name, _ in versions:
    d, h = times[name]
    md, mh = statistics.median(d), statistics.median(h)
    print("%-22s %12.1f %22s %9.2fx %14.1f %22s %9.2fx" % (name, md * 1e6, "[%.1f - %.1f]" % (min(d) * 1e6, max(d) * 1e6), base[0] / md,
                                                           mh * 1e6, "[%.1f - %.1f]" % (min(h) * 1e6, max(h) * 1e6), base[1] / mh))
md, mh = (statistics.median(x) for x in times["device adamw_step"])
print("# pass mark (adamw_step's median below the torch tail's in this run, on both clocks): %s" % ("met" if md < base[0] and mh < base[1] else "NOT met"))
