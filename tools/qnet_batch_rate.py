"""DeviceQNetwork.forward_batch and g2048.dqn_targets (the network work of DQNAgent.train_step's no-gradient block,
agents/hybrid.py:1038-1046) against stock torch on the same GPU.

    python3 tools/qnet_batch_rate.py

The reference's shape (dim_ff 2048, 2 layers, torch's default init) at n = 64, 256, 1,024 and 4,096 boards; 256 is the batch
train_step uses. Versions, alternating within every round:
  torch f32 eager / graph   the stock eval-mode module's own batch call (the encoder sees x.unsqueeze(1): one sequence of n
                            tokens), eager and replayed from a captured graph: the yardstick;
  device batch              DeviceQNetwork.forward_batch: the same function, 12 launches;
  device per-board          DeviceQNetwork.__call__, for context: a DIFFERENT function (every board its own sequence);
  torch targets / device targets   the whole of :1041-1046: two batch forwards and the three lines of torch, against
                            g2048.dqn_targets.
A round times REPS back-to-back calls of a version between one event pair and divides; median of 7 rounds after 2 warm-up rounds,
min - max in brackets. Before timing, the device Q-values and stock torch's float32 ones are both compared with the module in
float64 on the same GPU (the device must stay within 8 x torch's own float32 error, the tests' convention).
Output: one text table (profiles/r16_qnet_batch_rate.txt keeps a run)."""
import copy
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

ge.import_package()
import g2048  # noqa: E402
from g2048 import DeviceQNetwork, ops  # noqa: E402

dev = torch.device("cuda")
DIM_FF, LAYERS, REPS, GAMMA = 2048, 2, 20, 0.99


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


def event_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / REPS


def alternate(versions, warmup, rounds):
    """{name: [seconds per call and round]}: every round runs each version, in order."""
    times = {name: [] for name, _ in versions}
    for r in range(warmup + rounds):
        for name, fn in versions:
            dt = event_time(fn)
            if r >= warmup:
                times[name].append(dt)
    return times


def tile_values(boards):
    return torch.where(boards > 0, torch.ones_like(boards, dtype=torch.int64) << boards.to(torch.int64), 0).to(torch.float32)


torch.manual_seed(0)
online_m, target_m = QNet().to(dev).eval(), QNet().to(dev).eval()
online, target = DeviceQNetwork(online_m), DeviceQNetwork(target_m)
online_f64 = copy.deepcopy(online_m).double()

print("# dim_ff %d, %d layers; %d calls per event pair; median of 7 rounds after 2 warm-up rounds, the versions alternating" % (DIM_FF, LAYERS, REPS))
print("%-7s %-18s %10s %22s %12s %10s" % ("boards", "version", "us", "[min - max] us", "boards/s", "vs eager"))
for n in (64, 256, 1024, 4096):
    boards = ops.synth_boards(n, seed=3, device=dev)
    x = tile_values(boards)
    shaped = torch.linspace(-5, 20, n, device=dev)
    dones = (torch.arange(n, device=dev) % 5 == 0).to(torch.float32)
    with torch.no_grad():
        want = online_f64(x.double())
        err_torch = (online_m(x).double() - want).abs().max().item() / want.abs().max().item()
    err = (online.forward_batch(boards).double() - want).abs().max().item() / want.abs().max().item()
    print("# n = %d: max |dQ| against the module in f64, of max|Q| %.3g: device batch %.3g, torch f32 %.3g" % (n, want.abs().max().item(), err, err_torch))
    assert err <= 8 * err_torch, "forward_batch does not compute torch's function"

    def eager():
        with torch.no_grad():
            return online_m(x)

    def torch_targets():
        with torch.no_grad():
            next_actions = online_m(x).argmax(1, keepdim=True)
            next_q = target_m(x).gather(1, next_actions).squeeze(1)
            return shaped + (1 - dones) * GAMMA * next_q

    graph = torch.cuda.CUDAGraph()
    eager()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        eager()
    versions = [("torch f32 eager", eager), ("torch f32 graph", graph.replay), ("device batch", lambda: online.forward_batch(boards)),
                ("device per-board", lambda: online(boards)), ("torch targets", torch_targets),
                ("device targets", lambda: g2048.dqn_targets(online, target, boards, shaped, dones, GAMMA))]
    times = alternate(versions, 2, 7)
    for name, _ in versions:
        t = times[name]
        med = statistics.median(t)
        base = statistics.median(times["torch targets" if name.endswith("targets") else "torch f32 eager"])
        print("%-7d %-18s %10.1f %22s %12.4g %9.2fx" % (n, name, med * 1e6, "[%.1f - %.1f]" % (min(t) * 1e6, max(t) * 1e6), n / med, base / med))
    del graph
    torch.cuda.empty_cache()
