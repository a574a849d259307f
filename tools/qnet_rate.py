"""g2048_qnet_forward (the hybrid agent's CNN-transformer Q-network, agents/hybrid.py:700-727) against stock torch.

    python3 tools/qnet_rate.py [--quick]

The forward alone at the reference's shape (dim_ff 2048, 2 layers, 1,326,180 parameters, torch's default init) over a range of
batch sizes up to 262,144 boards (--quick: up to 65,536): stock torch f32 eager and replayed from a captured graph, computing
the same per-board function (the module in eval mode with the encoder input reshaped to (1, B, 128): every board its own
sequence of one token), DeviceQNetwork f32 and bf16. Event pairs after 2 warm-up rounds; the four versions alternate within
every round; median of 7 rounds with min - max. Stock torch above 65,536 boards runs as calls of 65,536. FLOP per board from the
shapes (what the device kernel executes: the V projection only), achieved TF and the share of the precision's MFMA peak (157.3
TF f32, 2.5 PF bf16); stock torch also computes Q and K (98,304 more MACs a board), which its rate is not credited with.
Before timing, the device Q-values are compared with torch's on the first boards.
Output: one text table (profiles/r10_qnet_rate.txt keeps a run)."""
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

ge.import_package()
from g2048 import DeviceQNetwork, ops  # noqa: E402

QUICK = "--quick" in sys.argv
dev = torch.device("cuda")
PEAK = {"f32": 157.3e12, "bf16": 2.5e15}
CHUNK = 65536
DIM_FF, LAYERS = 2048, 2


def flop_per_board(dim_ff=DIM_FF, layers=LAYERS):
    """2 x MACs: conv1, conv2, Linear(1024,128), per layer V, out_proj and the feed-forward pair, Linear(128,4)."""
    return 2 * (25 * 32 * 4 + 16 * 64 * 128 + 1024 * 128 + layers * (2 * 128 * 128 + 2 * 128 * dim_ff) + 128 * 4)


class QNet(nn.Module):                  # the reference's structure, stock torch, default init
    def __init__(self, dim_ff=DIM_FF, layers=LAYERS):
        super().__init__()
        self.cnn = nn.Sequential(nn.Conv2d(1, 32, kernel_size=2, stride=1, padding=1), nn.ReLU(),
                                 nn.Conv2d(32, 64, kernel_size=2, stride=1, padding=0), nn.ReLU())
        self.embedding = nn.Linear(1024, 128)
        self.transformer = nn.TransformerEncoder(nn.TransformerEncoderLayer(d_model=128, nhead=8, dim_feedforward=dim_ff), layers,
                                                 enable_nested_tensor=False)
        self.fc = nn.Linear(128, 4)

    def forward(self, x):               # per board: the encoder sees (1, B, 128), B sequences of one token
        h = self.embedding(self.cnn(x.view(-1, 1, 4, 4)).view(x.shape[0], -1))
        return self.fc(self.transformer(h.unsqueeze(0)).squeeze(0))


def event_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def alternate(versions, warmup, rounds):
    """{name: [seconds per round]}: every round runs each version once, in order."""
    times = {name: [] for name, _ in versions}
    for r in range(warmup + rounds):
        for name, fn in versions:
            dt = event_time(fn)
            if r >= warmup:
                times[name].append(dt)
    return times


torch.manual_seed(0)
net = QNet().to(dev).eval()
nets = {prec: DeviceQNetwork(net, precision=prec) for prec in ("f32", "bf16")}
print("# dim_ff %d, %d layers: %.3f MFLOP per board; packed weights f32 %.2f MB, bf16 %.2f MB" % (
    DIM_FF, LAYERS, flop_per_board() / 1e6, nets["f32"].packed.numel() / 1e6, nets["bf16"].packed.numel() / 1e6))

check = ops.synth_boards(4096, seed=3, device=dev)
tiles = torch.where(check > 0, torch.ones_like(check, dtype=torch.int64) << check.to(torch.int64), 0).to(torch.float32)
with torch.no_grad():
    want = net(tiles)
for prec in ("f32", "bf16"):
    err = (nets[prec](check) - want).abs().max().item() / want.abs().max().item()
    print("# device %s vs torch f32 on 4,096 boards: max |dQ| = %.3g of max|Q| %.3g" % (prec, err, want.abs().max().item()))
    assert err < (1e-4 if prec == "f32" else 5e-2), "the device kernel does not compute torch's function"

print("# forward alone (median of 7 rounds after 2 warm-up rounds, the versions alternating; min - max in brackets)")
print("%-9s %-18s %10s %22s %12s %8s %8s %10s" % ("boards", "version", "ms", "[min - max] ms", "boards/s", "TF", "of peak", "vs graph"))
for n in (256, 2048, 16384, 65536) if QUICK else (256, 2048, 16384, 65536, 262144):
    boards = ops.synth_boards(n, seed=3, device=dev)
    x = torch.where(boards > 0, torch.ones_like(boards, dtype=torch.int64) << boards.to(torch.int64), 0).to(torch.float32)
    parts = [x[i:i + CHUNK] for i in range(0, n, CHUNK)]

    def eager():
        with torch.no_grad():
            for part in parts:
                net(part)

    graph = torch.cuda.CUDAGraph()
    eager()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        eager()
    versions = [("torch f32 eager", eager), ("torch f32 graph", graph.replay),
                ("device f32", lambda: nets["f32"](boards)), ("device bf16", lambda: nets["bf16"](boards))]
    times = alternate(versions, 2, 7)
    base = statistics.median(times["torch f32 graph"])
    for name, _ in versions:
        t = times[name]
        med = statistics.median(t)
        prec = "bf16" if name.endswith("bf16") else "f32"
        tf = flop_per_board() * n / med
        print("%-9d %-18s %10.3f %22s %12.4g %8.1f %7.1f%% %9.2fx" % (n, name, med * 1e3, "[%.3f - %.3f]" % (min(t) * 1e3, max(t) * 1e3),
                                                                   n / med, tf / 1e12, 100 * tf / PEAK[prec], base / med))
    del graph, x, parts
    torch.cuda.empty_cache()
