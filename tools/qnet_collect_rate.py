"""Experience collection of the hybrid agent: g2048.DQNCollector.collect in ONE launch (g2048_qnet_collect) against the two baselines
made of the entry points that were there before it -- collect(fused=False), the same function one env step at a time, and the
hand-strung loop of examples/dqn_replay.py (--collector legacy).

    python3 tools/qnet_collect_rate.py [--envs 4096,65536] [--steps 16] [--rounds 5] [--dim-ff 2048] [--layers 2] [--out FILE]

Per case (envs x precision x beam off / on at the reference's 15 / 30 / 64): the three paths ALTERNATE within every round; a round
is `steps` env steps of every env into a ring that already holds a warm-up's transitions (200,000 entries, 2 Mi for more than
8,192 envs), timed with a device event pair (the host enqueues ahead: what is measured is the stream, not the interpreter, unless
the host is the slower of the two -- which is the stepwise paths' problem and is why the host clock round the same work, ending in
a synchronise, is printed too). One untimed warm-up round per path and case first. Median of the rounds with min - max, per ENV
STEP (the round's time / steps), and the transitions per second of the median. The legacy loop knows neither the beam search nor
the episode cap and is timed in the beam-off cases only.

Stream operations per env step (launches, memsets and copies enqueued on the stream; counted from the code, not measured):
    fused      3 per `steps` env steps (memset, per_max_kernel, qnet_collect_kernel)
    stepwise   22 with the episode cap on (the default 2000), 13 with max_episode_steps = 0: forward, select (act_beam: the same
               two), a clone of the scores, two env steps, three of the push, six elementwise for the counts and the masks, and
               with the cap nine more (the step of the finished boards, its zeroed scores, seven elementwise)
    legacy     14: a clone, forward, select, the env step and its `done`, three of the push, reset, three for the two
               torch.where, two copies of env.load
Writes one text table (profiles/r34_qnet_collect_rate.txt keeps a run)."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

ge.import_package()
import g2048  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", default="4096,65536")
ap.add_argument("--steps", type=int, default=16)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--dim-ff", type=int, default=2048)
ap.add_argument("--layers", type=int, default=2)
ap.add_argument("--epsilon", type=float, default=0.2)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("qnet_collect_rate: needs a GPU; a rate is a measurement on the device or nothing")
dev, SEED = torch.device("cuda"), 1
BEAM = dict(use_beam_search=True, beam_width=15, search_depth=30, threshold=64)
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


class HybridDQN(nn.Module):             # the reference's layout (agents/hybrid.py:700-727), stock torch, default init
    def __init__(self, dim_ff, layers):
        super().__init__()
        self.cnn = nn.Sequential(nn.Conv2d(1, 32, kernel_size=2, stride=1, padding=1), nn.ReLU(),
                                 nn.Conv2d(32, 64, kernel_size=2, stride=1, padding=0), nn.ReLU())
        self.embedding = nn.Linear(1024, 128)
        self.transformer = nn.TransformerEncoder(nn.TransformerEncoderLayer(d_model=128, nhead=8, dim_feedforward=dim_ff), layers,
                                                 enable_nested_tensor=False)
        self.fc = nn.Linear(128, 4)


class Legacy:
    """examples/dqn_replay.py's play(): a VecGame2048, act, env.step, push, a reset from the RESET domain and two torch.where."""

    def __init__(self, net, n, capacity):
        self.net, self.n, self.t = net, n, 0
        self.env = g2048.VecGame2048(n, device=dev, seed=SEED)
        self.buf = g2048.DeviceReplayBuffer(capacity, device=dev, seed=SEED)

    def collect(self, steps, epsilon):
        env, buf = self.env, self.buf
        for t in range(self.t, self.t + steps):
            state = env.boards.clone()
            actions, _ = self.net.act(state, epsilon=epsilon, seed=SEED, step_index=t)
            nxt, reward, done, _ = env.step(actions)
            buf.push(state, actions, reward, nxt, env.flags)
            fresh, _ = g2048.ops.reset(self.n, SEED, t + 1, 0, device=dev)
            env.load(torch.where(done[:, None], fresh, nxt), torch.where(done, torch.zeros_like(env.scores), env.scores))
        self.t += steps


def timed(fn):
    """(device seconds, host seconds) of fn(): an event pair on the stream, and the host clock round the same work and a synchronise."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e-3, time.perf_counter() - t0


def med(xs, steps):
    per = [x / steps * 1e3 for x in xs]
    return "%8.3f ms (%.3f - %.3f)" % (statistics.median(per), min(per), max(per))


torch.manual_seed(0)
model = HybridDQN(a.dim_ff, a.layers).to(dev).eval()
nets = {p: g2048.DeviceQNetwork(model, precision=p) for p in ("f32", "bf16")}
say("experience collection, HybridDQN dim_ff %d, %d layers, epsilon %.2f, %d env steps a round, %d rounds after one warm-up round a path;"
    % (a.dim_ff, a.layers, a.epsilon, a.steps, a.rounds))
say("per ENV STEP: median (min - max) of the rounds, device events | host clock to a synchronise | transitions/s of the device median")
say("stream operations per env step: fused 3 / %d, stepwise 22 (episode cap 2000 on), legacy 14" % a.steps)
for n in (int(v) for v in a.envs.split(",")):
    capacity = 200000 if n <= 8192 else 2 << 20
    for precision in ("f32", "bf16"):
        for beam in (False, True):
            kw = BEAM if beam else {}
            paths = {}
            for name, fused in (("fused", True), ("stepwise", False)):
                buf = g2048.DeviceReplayBuffer(capacity, device=dev, seed=SEED)
                col = g2048.DQNCollector(nets[precision], buf, n, seed=SEED, device=dev)
                paths[name] = lambda col=col, fused=fused: col.collect(a.steps, a.epsilon, fused=fused, **kw)
            if not beam:
                legacy = Legacy(nets[precision], n, capacity)
                paths["legacy"] = lambda legacy=legacy: legacy.collect(a.steps, a.epsilon)
            for fn in paths.values():            # warm-up: code objects, buffers, and a ring that is no longer empty
                fn()
            torch.cuda.synchronize()
            times = {name: [] for name in paths}
            for _ in range(a.rounds):
                for name, fn in paths.items():
                    times[name].append(timed(fn))
            say()
            say("%d envs, %s, beam %s, ring %d" % (n, precision, "15 / 30 / 64" if beam else "off", capacity))
            for name in paths:
                d, h = [t[0] for t in times[name]], [t[1] for t in times[name]]
                say("  %-9s %s | %s | %.3g transitions/s" % (name, med(d, a.steps), med(h, a.steps), n * a.steps / statistics.median(d)))
            f, s = statistics.median(t[0] for t in times["fused"]), statistics.median(t[0] for t in times["stepwise"])
            say("  fused against stepwise: %.2fx the device time (%s)" % (f / s, "faster" if f < s else "SLOWER"))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
