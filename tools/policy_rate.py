"""g2048_policy_forward on its own and inside RolloutCollector (BASELINE config 4: 65,536 envs x 128 steps).

    python3 tools/policy_rate.py [--quick]

(a) the forward alone at 65,536 and 1,048,576 boards, f32 / bf16, actor only / actor + critic: event pairs after warm-up,
    median of 7, FLOP/s against the 157.3 TF (f32 MFMA) / 2.5 PF (bf16 MFMA) peaks;
(b) RolloutCollector at 65,536 x 128 with bench.py's stock-torch ActorCritic, with DevicePolicy f32 / bf16 built from the same
    modules, and with the uniform policy (env side only); collect() after two warm-up collects (capture included), median of 5.
Output: one text table (profiles/r06_policy_rate.txt keeps a run)."""
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

ge.import_package()
from g2048 import DevicePolicy, RolloutCollector, ops  # noqa: E402

QUICK = "--quick" in sys.argv
dev = torch.device("cuda")
MAC = {4: 16 * 256 + 256 * 128 + 128 * 64 + 64 * 4, 1: 16 * 256 + 256 * 128 + 128 * 64 + 64 * 1}     # per board
PEAK = {"f32": 157.3e12, "bf16": 2.5e15}


class ActorCritic(nn.Module):           # bench.py's config-4 policy: the reference's MLP shapes, BatchNorm + ReLU, eval mode
    def __init__(self):
        super().__init__()

        def trunk():
            return nn.Sequential(nn.Linear(16, 256), nn.BatchNorm1d(256), nn.ReLU(), nn.Linear(256, 128), nn.BatchNorm1d(128),
                                 nn.ReLU(), nn.Linear(128, 64), nn.BatchNorm1d(64), nn.ReLU())
        self.actor, self.critic = nn.Sequential(trunk(), nn.Linear(64, 4)), nn.Sequential(trunk(), nn.Linear(64, 1))

    def forward(self, x):
        return torch.softmax(self.actor(x), -1), self.critic(x)


class Uniform(nn.Module):
    def forward(self, x):
        return torch.full((x.shape[0], 4), 0.25, device=x.device)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e-3)
    return statistics.median(out)


torch.manual_seed(0)
net = ActorCritic().to(dev).eval()
print("# g2048_policy_forward alone (one launch; median of 7 event pairs after 3 warm-up launches)")
print("%-9s %-6s %-14s %10s %14s %8s" % ("boards", "prec", "networks", "us", "boards/s", "of peak"))
for n in (65536, 1048576):
    boards = ops.synth_boards(n, seed=3, device=dev)
    for prec in ("f32", "bf16"):
        pol = DevicePolicy(net.actor, net.critic, precision=prec)
        for with_critic in (False, True):
            c = pol.critic.blob(n) if with_critic else None
            probs = torch.empty((n, 4), device=dev)
            value = torch.empty((n, 1), device=dev) if with_critic else None

            def run():
                ops.policy_forward(boards, pol.actor.blob(n), c, prec, probs=probs, value=value)
            for _ in range(3):
                run()
            torch.cuda.synchronize()
            dt = timed(run, 7)
            flop = 2.0 * n * (MAC[4] + (MAC[1] if with_critic else 0))
            print("%-9d %-6s %-14s %10.2f %14.4g %7.1f%%" % (n, prec, "actor+critic" if with_critic else "actor", dt * 1e6, n / dt,
                                                          100 * flop / dt / PEAK[prec]))

print()
print("# RolloutCollector, 65,536 envs x 128 steps, hipGraph replay per collect() (median of %d collects after 2 warm-up)" % (3 if QUICK else 5))
print("%-34s %12s %16s %10s" % ("policy", "ms/collect", "env-steps/s", "vs torch"))
base = None
for name, pol in (("torch ActorCritic (bench.py)", net), ("DevicePolicy f32", DevicePolicy(net.actor, net.critic, precision="f32")),
                  ("DevicePolicy bf16", DevicePolicy(net.actor, net.critic, precision="bf16")), ("uniform (env only)", Uniform())):
    rc = RolloutCollector(65536, 128, pol, device=dev, seed=0x2048)
    rc.collect()
    rc.collect()
    torch.cuda.synchronize()
    walls = []
    for _ in range(3 if QUICK else 5):
        t0 = time.perf_counter()
        rc.collect()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    dt = statistics.median(walls)
    rate = 65536 * 128 / dt
    base = base or rate
    print("%-34s %12.2f %16.4g %9.2fx" % (name, dt * 1e3, rate, rate / base))
