"""g2048_tpolicy_forward on its own and inside RolloutCollector (BASELINE config 4: 65,536 envs x 128 steps, transformer policy).

    python3 tools/tpolicy_rate.py [--quick]

(a) the forward alone at 65,536 and 1,048,576 boards, dim_ff 128 (bench.py's shape) and 2048 (the reference's default): stock
    torch f32 eager, stock torch f32 replayed from a captured graph (what RolloutCollector does with it), DeviceTransformerPolicy
    f32 and bf16. Event pairs after 2 warm-up rounds; the four versions alternate within every round; median of 7 rounds with
    min - max. Stock torch at 1,048,576 boards runs as 16 calls of 65,536 (its dim_ff 2048 activations would take 137 GB in
    one call). FLOP per board from the shapes, achieved TF and the share of the precision's MFMA peak (157.3 TF f32, 2.5 PF bf16).
(b) RolloutCollector(65536, 128) end to end at dim_ff 128 with the same four policies, alternating, median of 5 collects
    with min - max after 2 warm-up collects each (capture included).
Output: one text table (profiles/r08_tpolicy_rate.txt keeps a run)."""
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

ge.import_package()
from g2048 import DeviceTransformerPolicy, RolloutCollector, ops  # noqa: E402

QUICK = "--quick" in sys.argv
dev = torch.device("cuda")
PEAK = {"f32": 157.3e12, "bf16": 2.5e15}
CHUNK = 65536


def flop_per_board(dim_ff, layers=2):
    """2 x MACs: per layer QKV, Q K^T, P V, out_proj, the feed-forward pair; then fc1, fc2 and the two heads."""
    per_token = 3 * 64 * 64 + 64 * 64 + 2 * 64 * dim_ff
    attention = 2 * 4 * 16 * 16 * 16                           # 4 heads x (16 x 16 x 16) x 2 products
    return 2 * (layers * (16 * per_token + attention) + 1024 * 128 + 128 * 64 + 64 * 5)


class Policy(nn.Module):                # bench.py's config-4 transformer: models/transformer.py's shape, stock torch, random init
    def __init__(self, dim_ff):
        super().__init__()
        self.emb = nn.Linear(1, 64)
        self.enc = nn.TransformerEncoder(nn.TransformerEncoderLayer(64, 4, dim_ff, batch_first=True), 2)
        self.fc = nn.Sequential(nn.Linear(1024, 128), nn.ReLU(), nn.Linear(128, 64), nn.ReLU())
        self.actor, self.critic = nn.Linear(64, 4), nn.Linear(64, 1)

    def forward(self, x):
        h = self.fc(self.enc(self.emb(x.view(x.shape[0], 16, 1))).reshape(x.shape[0], -1))
        return torch.softmax(self.actor(h), -1), self.critic(h)


def event_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def alternate(versions, warmup, rounds, measure):
    """{name: [seconds per round]}: every round runs each version once, in order."""
    times = {name: [] for name, _ in versions}
    for r in range(warmup + rounds):
        for name, fn in versions:
            dt = measure(fn)
            if r >= warmup:
                times[name].append(dt)
    return times


def wall_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


print("# flop per board: dim_ff 128: %.3f MFLOP, dim_ff 2048: %.3f MFLOP" % (flop_per_board(128) / 1e6, flop_per_board(2048) / 1e6))
print("# forward alone (median of 7 rounds after 2 warm-up rounds, the versions alternating; min - max in brackets)")
print("%-8s %-9s %-22s %10s %22s %12s %8s %8s" % ("dim_ff", "boards", "version", "ms", "[min - max] ms", "boards/s", "TF", "of peak"))
torch.manual_seed(0)
nets = {ff: Policy(ff).to(dev).eval() for ff in (128, 2048)}
for ff in (128, 2048):
    net = nets[ff]
    pols = {prec: DeviceTransformerPolicy(net, precision=prec) for prec in ("f32", "bf16")}
    for n in (65536,) if QUICK else (65536, 1048576):
        boards = ops.synth_boards(n, seed=3, device=dev)
        obs = boards.to(torch.float32) / 15
        parts = [obs[i:i + CHUNK] for i in range(0, n, CHUNK)]

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
                    ("device f32", lambda: pols["f32"](boards)), ("device bf16", lambda: pols["bf16"](boards))]
        times = alternate(versions, 2, 7, event_time)
        for name, _ in versions:
            t = times[name]
            med = statistics.median(t)
            prec = "bf16" if name.endswith("bf16") else "f32"
            tf = flop_per_board(ff) * n / med
            print("%-8d %-9d %-22s %10.3f %22s %12.4g %8.1f %7.1f%%" % (ff, n, name, med * 1e3, "[%.3f - %.3f]" % (min(t) * 1e3, max(t) * 1e3),
                                                                  n / med, tf / 1e12, 100 * tf / PEAK[prec]))
        del graph, obs, parts
        torch.cuda.empty_cache()

rounds = 3 if QUICK else 5
print()
print("# RolloutCollector, 65,536 envs x 128 steps, dim_ff 128 (median of %d collects after 2 warm-up, the versions alternating)" % rounds)
print("%-34s %12s %24s %16s %10s" % ("policy", "ms/collect", "[min - max] ms", "env-steps/s", "vs torch"))
net = nets[128]
setups = [("torch f32, eager loop", net, False), ("torch f32, hipGraph", net, True),
          ("DeviceTransformerPolicy f32", DeviceTransformerPolicy(net, precision="f32"), True),
          ("DeviceTransformerPolicy bf16", DeviceTransformerPolicy(net, precision="bf16"), True)]
collectors = [(name, RolloutCollector(65536, 128, pol, device=dev, seed=0x2048, use_graph=g).collect) for name, pol, g in setups]
times = alternate(collectors, 2, rounds, wall_time)
base = statistics.median(times["torch f32, hipGraph"])
for name, _ in collectors:
    t = times[name]
    med = statistics.median(t)
    print("%-34s %12.2f %24s %16.4g %9.2fx" % (name, med * 1e3, "[%.2f - %.2f]" % (min(t) * 1e3, max(t) * 1e3), 65536 * 128 / med, base / med))
