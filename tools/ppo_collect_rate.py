"""PPO experience collection: g2048.RolloutCollector(sampler="collect"), the whole collect in ONE launch (g2048_ppo_collect), against
sampler="fused" with hipGraph replay, the path that was there before it: g2048_policy_forward + g2048_rollout_step per env step,
2 x steps kernels a collect replayed from one graph.

    python3 tools/ppo_collect_rate.py [--envs 4096,65536] [--steps 128] [--rounds 5] [--out FILE]

Per case (envs x precision x actor only / actor + critic) both collectors are built from the same modules with the same seed. Two
untimed warm-up collects each (the graph's capture included), then the two paths ALTERNATE within every round; a collect is timed
with a device event pair. Median of the rounds with min - max, per collect and per env step, and the env steps per second of the
median. Before the rounds the first collect of both is compared: the trajectories are the same bits, or the case says DIFFERENT.
`uniform (env only)` is sampler="fused" with a policy that returns 0.25 everywhere: the env half of a step alone, for scale.
Kernels a collect: collect 1 (+ torch's log and the counter's add), fused 2 x steps + the same log, replayed from a graph.
Writes one text table (profiles/r35_ppo_collect_rate.txt keeps a run)."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

ge.import_package()
from g2048 import DevicePolicy, RolloutCollector  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", default="4096,65536")
ap.add_argument("--steps", type=int, default=128)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("ppo_collect_rate: needs a GPU; a rate is a measurement on the device or nothing")
dev, SEED = torch.device("cuda"), 0x2048
COMPARED = ("obs", "valid_mask", "actions", "log_prob", "values", "rewards", "dones", "last_obs")
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def net(n_out):                         # bench.py's config-4 halves: the reference's MLP shapes, BatchNorm + ReLU, eval mode
    trunk = nn.Sequential(nn.Linear(16, 256), nn.BatchNorm1d(256), nn.ReLU(), nn.Linear(256, 128), nn.BatchNorm1d(128), nn.ReLU(),
                          nn.Linear(128, 64), nn.BatchNorm1d(64), nn.ReLU())
    return nn.Sequential(trunk, nn.Linear(64, n_out))


class Uniform(nn.Module):
    def forward(self, x):
        return torch.full((x.shape[0], 4), 0.25, device=x.device)


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e-3


def row(name, times, n):
    ms = [t * 1e3 for t in times]
    m = statistics.median(ms)
    say("  %-20s %8.3f ms (%.3f - %.3f) a collect | %7.2f us a step | %.4g env-steps/s"
        % (name, m, min(ms), max(ms), m / a.steps * 1e3, n * a.steps / (m * 1e-3)))
    return m


torch.manual_seed(0)
actor, critic = net(4).to(dev).eval(), net(1).to(dev).eval()
say("PPO experience collection, %d steps a collect, %d rounds after 2 warm-up collects a path, the paths alternating within a round;"
    % (a.steps, a.rounds))
say("per collect: median (min - max) of the rounds, device events | per env step | env steps/s of the median")
for n in (int(v) for v in a.envs.split(",")):
    uniform = RolloutCollector(n, a.steps, Uniform(), device=dev, seed=SEED)
    for precision in ("f32", "bf16"):
        for with_critic in (False, True):
            pol = DevicePolicy(actor, critic if with_critic else None, precision=precision)
            cols = {"collect": RolloutCollector(n, a.steps, pol, device=dev, seed=SEED, sampler="collect"),
                    "fused (graph)": RolloutCollector(n, a.steps, pol, device=dev, seed=SEED, sampler="fused")}
            first = {name: {k: v.clone() for k, v in col.collect().items() if k in COMPARED} for name, col in cols.items()}
            same = all(torch.equal(first["collect"][k].view(torch.uint8), first["fused (graph)"][k].view(torch.uint8)) for k in COMPARED)
            del first
            for col in list(cols.values()) + [uniform]:
                col.collect()
            torch.cuda.synchronize()
            assert cols["fused (graph)"]._graph is not None, "the fused collector did not capture its loop"
            cols["uniform (env only)"] = uniform
            times = {name: [] for name in cols}
            for _ in range(a.rounds):
                for name, col in cols.items():
                    times[name].append(timed(col.collect))
            say()
            say("%d envs, %s, %s; first collects: %s" % (n, precision, "actor + critic" if with_critic else "actor only",
                                                       "the same bits" if same else "DIFFERENT"))
            med = {name: row(name, times[name], n) for name in cols}
            c, f = med["collect"], med["fused (graph)"]
            say("  collect against fused: %.2fx the device time (%s)" % (c / f, "faster" if c < f else "SLOWER"))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
