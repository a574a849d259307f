"""A sample + update_priorities round of the prioritized replay buffer at the reference's own shape: 200,000 entries, batch 256
(DQNAgent's default) and batch 128 (what the reference's main() sets), g2048.DeviceReplayBuffer against a NumPy restatement of the
reference's buffer on the host (agents/hybrid.py:730-765: two deques, np.array over the priorities deque, np.random.choice(p=...), a
Python loop over the updated indices).

    python3 tools/per_rate.py [--entries 200000] [--rounds 20]

The device side is timed with an event pair around `rounds` rounds (sample, then update_priorities with the sampled indices) and
also by the host clock around the same work ending in a synchronise; the host side by the host clock (it enqueues nothing). The
two sides alternate within every repeat; median of 5 repeats with min - max. The device round includes what the reference does
after sample() in train_step (:961-969 the tensors, :971-1034 the reward shaping); the host round does not. Also one push of 4,096
transitions into the full ring (the maximum over 200,000 priorities, then the scatter).
Output: one text table (profiles/r15_per_rate.txt keeps a run)."""
import argparse
import collections
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

ge.import_package()
from g2048 import DeviceReplayBuffer, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--entries", type=int, default=200000)
ap.add_argument("--rounds", type=int, default=20)
a = ap.parse_args()
dev = torch.device("cuda")
N, ALPHA, BETA = a.entries, 0.6, 0.4


class HostBuffer:
    """The reference's buffer restated: deques of transitions and priorities."""

    def __init__(self, capacity, alpha):
        self.buffer, self.priorities, self.alpha = collections.deque(maxlen=capacity), collections.deque(maxlen=capacity), alpha

    def push(self, transition):
        self.priorities.append(max(self.priorities, default=1.0))
        self.buffer.append(transition)

    def sample(self, batch, beta):
        probs = np.array(self.priorities, dtype=np.float32) ** self.alpha
        probs /= probs.sum()
        indices = np.random.choice(len(self.buffer), batch, p=probs)
        samples = [self.buffer[i] for i in indices]
        weights = (len(self.buffer) * probs[indices]) ** (-beta)
        return samples, indices, weights / weights.max()

    def update_priorities(self, indices, priorities):
        for i, v in zip(indices, priorities):
            if i < len(self.priorities):
                self.priorities[i] = max(v, 1e-5)


def med(xs):
    return "%9.1f us (%.1f - %.1f)" % (statistics.median(xs) * 1e6, min(xs) * 1e6, max(xs) * 1e6)


rng = np.random.default_rng(1)
boards = ops.synth_boards(N, seed=1, device=dev)
nxt = ops.synth_boards(N, seed=2, device=dev)
acts = ops.synth_actions(N, seed=1, device=dev)
prio = torch.from_numpy(rng.exponential(1.0, N).astype(np.float32))
dbuf = DeviceReplayBuffer(N, alpha=ALPHA, device=dev, seed=1)
dbuf.push(boards, acts, torch.zeros(N, device=dev), nxt, torch.zeros(N, dtype=torch.uint8, device=dev))
dbuf.update_priorities(torch.arange(N, device=dev), prio.to(dev))
hbuf = HostBuffer(N, ALPHA)
state = np.zeros(16, np.float32)
hbuf.buffer.extend((state, 0, 0.0, state, False) for _ in range(N))
hbuf.priorities.extend((prio.numpy() + np.float32(1e-5)).tolist())
print("prioritized replay, %d entries, alpha %.1f, beta %.1f; %d rounds per timing, 5 repeats, the sides alternating" % (N, ALPHA, BETA, a.rounds))
for batch in (256, 128):
    td_dev = torch.from_numpy(rng.exponential(1.0, batch).astype(np.float32)).to(dev)
    td_host = td_dev.cpu().numpy()

    def device_rounds():
        for _ in range(a.rounds):
            res = dbuf.sample(batch, beta=BETA)
            dbuf.update_priorities(res[1], td_dev)

    def host_rounds(k):
        for _ in range(k):
            _, idx, _ = hbuf.sample(batch, BETA)
            hbuf.update_priorities(idx, td_host + np.float32(1e-5))

    device_rounds()
    torch.cuda.synchronize()
    ev, wall, hst = [], [], []
    host_k = max(1, a.rounds // 10)
    for rep in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        device_rounds()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) / a.rounds)
        ev.append(e0.elapsed_time(e1) * 1e-3 / a.rounds)
        t0 = time.perf_counter()
        host_rounds(host_k)
        hst.append((time.perf_counter() - t0) / host_k)
    print("batch %3d  device round, event pair   %s" % (batch, med(ev)))
    print("batch %3d  device round, host clock   %s" % (batch, med(wall)))
    print("batch %3d  host NumPy round           %s   = %.0f x the device round (event pair)" % (
        batch, med(hst), statistics.median(hst) / statistics.median(ev)), flush=True)
m = 4096
ev = []
flags = torch.zeros(m, dtype=torch.uint8, device=dev)
rew = torch.zeros(m, device=dev)
for rep in range(7):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    dbuf.push(boards[:m], acts[:m], rew, nxt[:m], flags)
    e1.record()
    torch.cuda.synchronize()
    ev.append(e0.elapsed_time(e1) * 1e-3)
print("push of %d into the full ring, event pair %s" % (m, med(ev[2:])))
