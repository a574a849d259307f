#!/usr/bin/env python3
"""Golden vectors of the hybrid agent's beam search: runs the REFERENCE's own DQNAgent.beam_search (agents/hybrid.py:814-907) and
records what it decided.

Usage (needs a checkout of the reference; the tests never read it, only the file this writes):

    python tests/golden/gen_qnet_beam_golden.py <reference checkout>

The agent is the reference's DQNAgent around HybridDQN().eval() in float32 on the weights of tests/qnet_weights.py, its env the
agent's own patched Game2048Env with env.board set to the tiles and state = env.get_state(). random.sample is replaced by
recorded draws through the oracle's sample_picks: pick j of the simulate_move call for action a uses draw (SEED, SIMULATE, step
index, board id, 3 a + j). The model is wrapped only to record what it returned. It writes qnet_beam.npz here (data only):

  seed, gamma, threshold
  d30_board (N,16)             uint8 codes: the planned boards of policy.npz, then synthetic ones (dead boards, full boards with
                               merges, fewer than 8 tiles, max below 64, tiles up to 2 ** 17)
  d30_planned (N,)             1 where beam_search planned (it called simulate_move), 0 where it took the argmax of Q
  d30_widths (7,)              1, 2, 4, 8, 15, 24, 30
  d30_action (7,N)             beam_search's action at search_depth 30 and that width; 255 where not planned
  d1_board (M,16)              planned boards of policy.npz
  d1_steps (2,), d1_widths (2,)  the two draw sets' step indices; 15, 4
  d1_h (2,M,4,3)               uint32: the draws of board i (id = i) in draw set s
  d1_succ (2,M,32,16)          the candidate boards simulate_move returned, slot 8 a + j; zero where unused
  d1_count (2,M,4)             transitions per action
  d1_leaf (2,M,32)             float32: model(candidate).max() exactly as the reference computed it, slot 8 a + j
  d1_action (2,2,M)            [draw set][width] beam_search's action at search_depth 1
  d1_action_d30 (2,M)          [width] the same boards at search_depth 30

It asserts the conditions that make the fixture pin something (see check_* below) and that the file is no larger than qnet.npz.

The committed file (this script is its only description; the table in README.md here has no row for it): N = 3,695 boards at
depth 30, 3,376 of them planned; M = 256 at depth 1, where 61 % of the decisions differ from depth 30, 8 boards change between the
draw sets and 20 decisions are an invalid move.
"""
import contextlib
import io
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2:
    sys.exit(__doc__)
REF = sys.argv[1]
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)
import qnet_weights as qw  # noqa: E402
from oracle import oracle as O  # noqa: E402
with contextlib.redirect_stdout(io.StringIO()):
    import agents.hybrid as hyb  # noqa: E402

SEED = 0x2048
D30_WIDTHS = (1, 2, 4, 8, 15, 24, 30)
D1_WIDTHS = (15, 4)
D1_STEPS = (5, 11)
D1_BOARDS = 256


def tiles_of(codes):
    c = np.asarray(codes, dtype=np.int64)
    return np.where(c > 0, 1 << c, 0).astype(np.int64)


def codes_of(tiles):
    t = np.asarray(tiles, dtype=np.int64).reshape(-1)
    c = np.zeros(t.shape, dtype=np.uint8)
    c[t > 0] = np.round(np.log2(t[t > 0])).astype(np.uint8)
    assert np.array_equal(tiles_of(c), t)
    return c


def hashed(step, ident, ctr):
    k0, k1 = O.rng_keys(SEED, O.DOM_SIMULATE, step)
    return O.rng_draw(k0, k1, ident, ctr)


class Recorder:
    """The agent with its env's simulate_move, its model and random.sample observed; one decide() per decision."""

    def __init__(self):
        torch.manual_seed(0)
        shapes = [(k, tuple(v.shape)) for k, v in hyb.HybridDQN().state_dict().items()]
        assert shapes == qw.reference_shapes()
        sd = {k: torch.from_numpy(v).float() for k, v in qw.state_dict(shapes).items()}
        model, target = hyb.HybridDQN().eval(), hyb.HybridDQN().eval()
        model.load_state_dict(sd)
        self.env = hyb.Game2048Env()
        with contextlib.redirect_stdout(io.StringIO()):
            self.agent = hyb.DQNAgent(self.env, model, target, hyb.PrioritizedReplayBuffer(16))
        assert (self.agent.beam_width, self.agent.search_depth, self.agent.use_beam_search, self.agent.beam_search_threshold,
                self.agent.gamma) == (15, 30, True, 64, 0.99)
        self.agent.device = torch.device("cpu")
        model.to("cpu").eval()
        real_sim = self.env.simulate_move

        def simulate_move(board, action):
            self.action, self.slot = int(action), 0
            res = real_sim(board, action)
            self.calls += 1
            self.count[action] = len(res)
            for j, (st, _, _) in enumerate(res):
                self.succ[8 * action + j] = codes_of(st)
            return res
        self.env.simulate_move = simulate_move

        def observed_model(x):
            out = model(x)
            if self.calls:             # a leaf of the search (the un-planned branch calls the model before any simulate_move)
                slot = 8 * self.action + self.slot
                assert np.array_equal(codes_of(x.numpy().reshape(-1)), self.succ[slot])
                self.leaf[slot] = out.max().numpy().astype(np.float32)
                self.slot += 1
                self.forwards += 1
            return out
        self.agent.model = observed_model

        def sample(population, k):
            picks = O.sample_picks(self.h[self.action], len(population))
            assert len(picks) == k
            return [population[i] for i in picks]
        random.sample = sample

    def decide(self, codes, width, depth, h):
        self.h, self.calls, self.forwards = h, 0, 0
        self.count = np.zeros(4, np.uint8)
        self.succ = np.zeros((32, 16), np.uint8)
        self.leaf = np.zeros(32, np.float32)
        self.env.board = tiles_of(codes).reshape(4, 4).copy()
        self.env.game_over = False
        self.agent.beam_width, self.agent.search_depth = width, depth
        return int(self.agent.beam_search(self.env.get_state()))


def synthetic_boards():
    rng = np.random.default_rng(20481)

    def rand(n, p_empty, max_code):
        b = rng.integers(1, max_code + 1, size=(n, 16)).astype(np.uint8)
        b[rng.random((n, 16)) < p_empty] = 0
        return b
    checker = np.array([[(1 + (r + c) % 2) for c in range(4)] for r in range(4)], np.uint8).reshape(16)
    dead = np.stack([checker + k for k in range(0, 14)] + [np.where(checker == 1, 6 + k, 3 + (k % 3)).astype(np.uint8) for k in range(10)])
    full = rand(260, 0.0, 9)                          # full boards, most with merges
    rows = rand(120, 0.0, 8)
    rows[:, 4:8] = rows[:, 0:4]                       # full boards whose UP / DOWN merge a whole row
    one_way = rand(160, 0.0, 11)
    one_way[:, [3, 7, 11, 15]] = 0                    # only RIGHT moves unless a row merges
    few = rand(150, 0.7, 10)                          # mostly fewer than 8 tiles
    low = rand(150, 0.3, 5)                           # max below 64
    big = rand(300, 0.35, 17)
    mid = rand(400, 0.3, 11)
    stacked = np.sort(rand(160, 0.25, 12), axis=1)[:, ::-1]       # monotone boards: RIGHT and DOWN change little or nothing
    stacked_t = np.ascontiguousarray(stacked.reshape(-1, 4, 4).transpose(0, 2, 1)).reshape(-1, 16)
    out = np.concatenate([dead, full, rows, one_way, few, low, big, mid, stacked, stacked[:, ::-1], stacked_t, stacked_t[:, ::-1]])
    out[out.max(axis=1) == 0, 5] = 1
    return np.ascontiguousarray(out.astype(np.uint8))


def gen_depth30(rec, policy_boards):
    import qnet_beam_ref as R
    pl = np.array([R.planned(b) for b in policy_boards])
    boards = np.concatenate([policy_boards[pl], synthetic_boards()])
    n = len(boards)
    planned = np.zeros(n, np.uint8)
    action = np.full((len(D30_WIDTHS), n), 255, np.uint8)
    ncand = np.zeros(n, np.int64)
    ties = 0
    for i, b in enumerate(boards):
        h = np.array([[hashed(0, i, 3 * a + j) for j in range(3)] for a in range(4)], np.uint32)
        for wi, w in enumerate(D30_WIDTHS):
            a = rec.decide(b, w, 30, h)
            if rec.calls == 0:
                break
            assert rec.calls == 4 and rec.forwards == 0, (rec.calls, rec.forwards)
            planned[i], action[wi, i], ncand[i] = 1, a, int(rec.count.sum())
        if planned[i]:                                # a tie at the top: the two best per-action sums are equal at width 30
            keys = sorted(((r * p, a) for a, r, p in R.candidates(b)), key=lambda t: -t[0])
            sums = {}
            for k, a in keys:
                sums[a] = sums.get(a, 0.0) + k
            s = sorted(sums.values(), reverse=True)
            ties += len(s) > 1 and s[0] == s[1]
    p = planned.astype(bool)
    counts = np.bincount(action[:, p].reshape(-1), minlength=4)
    print("depth 30: %d boards, %d planned; action counts over widths %s; top ties %d; < 24 candidates %d; exactly 4: %d" % (
        n, p.sum(), counts.tolist(), ties, (ncand[p] < 24).sum(), (ncand[p] == 4).sum()))
    assert 2500 <= n <= 4000
    assert (counts[:4] >= 10).all(), counts
    assert ties >= 0.25 * p.sum(), (ties, p.sum())
    assert (ncand[p] < 24).sum() >= 0.20 * p.sum()
    assert (ncand[p] == 4).sum() >= 10
    assert (~p).sum() >= 100 and np.array_equal(p, np.array([R.planned(b) for b in boards]))
    return dict(d30_board=boards, d30_planned=planned, d30_widths=np.array(D30_WIDTHS, np.int64), d30_action=action)


def gen_depth1(rec, policy_boards, m):
    import qnet_beam_ref as R
    boards = policy_boards[np.array([R.planned(b) for b in policy_boards])][:m]
    assert len(boards) == m
    H = np.zeros((2, m, 4, 3), np.uint32)
    succ = np.zeros((2, m, 32, 16), np.uint8)
    count = np.zeros((2, m, 4), np.uint8)
    leaf = np.zeros((2, m, 32), np.float32)
    action = np.zeros((2, 2, m), np.uint8)
    action30 = np.zeros((2, m), np.uint8)
    invalid = 0
    for i, b in enumerate(boards):
        for wi, w in enumerate(D1_WIDTHS):
            action30[wi, i] = rec.decide(b, w, 30, H[0, i])
        for s, step in enumerate(D1_STEPS):
            H[s, i] = [[hashed(step, i, 3 * a + j) for j in range(3)] for a in range(4)]
            for wi, w in enumerate(D1_WIDTHS):
                a = rec.decide(b, w, 1, H[s, i])
                assert rec.calls == 4 and rec.forwards == int(rec.count.sum())
                if wi:
                    assert np.array_equal(succ[s, i], rec.succ) and np.array_equal(leaf[s, i], rec.leaf)
                succ[s, i], count[s, i], leaf[s, i], action[s, wi, i] = rec.succ, rec.count, rec.leaf, a
                invalid += rec.count[a] == 1
    differs = (action != action30[None]).mean()
    changes = int((action[0] != action[1]).any(axis=0).sum())
    print("depth 1: %d boards; differs from depth 30 on %.1f %%; changes between the draw sets on %d boards; invalid move chosen %d times"
          % (m, 100 * differs, changes, invalid))
    ok = differs >= 0.25 and changes >= 2 and invalid >= 1
    return ok, dict(d1_board=boards, d1_steps=np.array(D1_STEPS, np.uint64), d1_widths=np.array(D1_WIDTHS, np.int64), d1_h=H,
                    d1_succ=succ, d1_count=count, d1_leaf=leaf, d1_action=action, d1_action_d30=action30)


def main():
    torch.set_num_threads(1)
    policy_boards = np.load(os.path.join(HERE, "policy.npz"))["boards"]
    real_sample = random.sample
    rec = Recorder()
    try:
        out = dict(seed=np.uint64(SEED), gamma=np.float64(rec.agent.gamma), threshold=np.int64(rec.agent.beam_search_threshold))
        out.update(gen_depth30(rec, policy_boards))
        m = D1_BOARDS
        while True:                                   # a missed condition enlarges the pool, never lowers the condition
            ok, d1 = gen_depth1(rec, policy_boards, m)
            if ok:
                break
            assert m < 1024, "the depth-1 conditions are not met by 1,024 boards"
            m *= 2
        out.update(d1)
    finally:
        random.sample = real_sample
    path = os.path.join(HERE, "qnet_beam.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "qnet.npz")), "qnet_beam.npz must not exceed qnet.npz"


if __name__ == "__main__":
    main()
