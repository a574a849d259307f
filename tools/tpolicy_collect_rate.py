"""The transformer policy's experience collection: g2048.RolloutCollector(sampler="collect") with a g2048.DeviceTransformerPolicy, the
whole collect in ONE launch (g2048_tpolicy_collect), against sampler="fused" with hipGraph replay, the path that was there before
it: g2048_tpolicy_forward + g2048_rollout_step per env step, 2 x steps kernels a collect replayed from one graph.

    python3 tools/tpolicy_collect_rate.py [--envs 256,1024,4096,65536] [--dim-ff 128,2048] [--steps 128] [--heavy-steps 16]
                                          [--rounds 5] [--out FILE]

Per case (envs x precision x dim_ff; 2 layers) both collectors are built from the same module with the same seed. The first
collect of both is compared and the case ASSERTS that the trajectories are the same bits. Then two untimed warm-up collects each
(the graph's capture included) and the two paths ALTERNATE within every round; a collect is timed with a device event pair. Median
of the rounds with min - max, per collect and per env step, and the env steps per second of the median. The heaviest case (the
largest --envs x f32 x dim_ff 2,048, where a step is tens of milliseconds) runs --heavy-steps steps a collect instead of --steps.
Kernels a collect: collect 1 (+ torch's log and the counter's add), fused 2 x steps + the same log + two row copies, replayed from
a graph. Writes one text table (profiles/r36_tpolicy_collect_rate.txt keeps a run)."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

ge.import_package()
from g2048 import DeviceTransformerPolicy, RolloutCollector  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", default="256,1024,4096,65536")
ap.add_argument("--dim-ff", default="128,2048")
ap.add_argument("--steps", type=int, default=128)
ap.add_argument("--heavy-steps", type=int, default=16)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("tpolicy_collect_rate: needs a GPU; a rate is a measurement on the device or nothing")
dev, SEED, LAYERS = torch.device("cuda"), 0x2048, 2
COMPARED = ("obs", "valid_mask", "actions", "log_prob", "values", "rewards", "dones", "last_obs")
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


class TransformerModel(nn.Module):      # the reference's layout (models/transformer.py:4-40), stock torch, default init
    def __init__(self, dim_ff):
        super().__init__()
        self.embedding = nn.Linear(1, 64)
        layer = nn.TransformerEncoderLayer(d_model=64, nhead=4, dim_feedforward=dim_ff, batch_first=True)
        self.transformer_encoder = nn.TransformerEncoder(layer, num_layers=LAYERS)
        self.fc1, self.fc2 = nn.Linear(1024, 128), nn.Linear(128, 64)
        self.actor, self.critic = nn.Linear(64, 4), nn.Linear(64, 1)


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e-3


def row(name, times, n, steps):
    ms = [t * 1e3 for t in times]
    m = statistics.median(ms)
    say("  %-16s %10.3f ms (%.3f - %.3f) a collect | %9.2f us a step | %.4g env-steps/s"
        % (name, m, min(ms), max(ms), m / steps * 1e3, n * steps / (m * 1e-3)))
    return m


sizes, widths = [int(v) for v in a.envs.split(",")], [int(v) for v in a.dim_ff.split(",")]
say("transformer-policy experience collection, %d layers, %d steps a collect (%d in the heaviest case), %d rounds after 2 warm-up"
    % (LAYERS, a.steps, a.heavy_steps, a.rounds))
say("collects a path, the paths alternating within a round; per collect: median (min - max) of the rounds, device events | per env")
say("step | env steps/s of the median. Every case first asserted that both paths' first collects are the same bits.")
for dim_ff in widths:
    torch.manual_seed(0)
    model = TransformerModel(dim_ff).to(dev).eval()
    for precision in ("f32", "bf16"):
        pol = DeviceTransformerPolicy(model, precision=precision)
        for n in sizes:
            heavy = n == max(sizes) and n >= 65536 and precision == "f32" and dim_ff >= 2048
            steps = a.heavy_steps if heavy else a.steps
            cols = {"collect": RolloutCollector(n, steps, pol, device=dev, seed=SEED, sampler="collect"),
                    "fused (graph)": RolloutCollector(n, steps, pol, device=dev, seed=SEED, sampler="fused")}
            first = {name: {k: v.clone() for k, v in col.collect().items() if k in COMPARED} for name, col in cols.items()}
            for k in COMPARED:
                assert torch.equal(first["collect"][k].view(torch.uint8), first["fused (graph)"][k].view(torch.uint8)), \
                    "%d envs, %s, dim_ff %d: %s of the first collects differs between the two paths" % (n, precision, dim_ff, k)
            del first
            for _ in range(2):
                for col in cols.values():
                    col.collect()
            torch.cuda.synchronize()
            assert cols["fused (graph)"]._graph is not None, "the fused collector did not capture its loop"
            times = {name: [] for name in cols}
            for _ in range(a.rounds):
                for name, col in cols.items():
                    times[name].append(timed(col.collect))
            say()
            say("%d envs, %s, dim_ff %d, %d steps; first collects: the same bits" % (n, precision, dim_ff, steps))
            med = {name: row(name, times[name], n, steps) for name in cols}
            c, f = med["collect"], med["fused (graph)"]
            say("  collect against fused: %.3fx the device time (%s)" % (c / f, "faster" if c < f else "SLOWER"))
            del cols
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
