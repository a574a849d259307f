#!/usr/bin/env python3
"""Golden vectors of the hybrid agent's prioritized replay: runs the REFERENCE's own PrioritizedReplayBuffer
(agents/hybrid.py:730-765) and DQNAgent.train_step (:955-1074) and records what they returned.

Usage (needs a checkout of the reference; the tests never read it, only the file this writes):

    python tests/golden/gen_per_golden.py <reference checkout>

It writes per.npz here (data only). This docstring is the file's only description: the table in README.md here has no row for it.

Shaping. The real train_step runs on batches of 256 handed to it by a stub buffer, around a small linear model (the shaping does
not read the network). Every transition is marked done, so the target train_step hands to nn.SmoothL1Loss (observed by a wrapper
that calls the real loss) is shaped_rewards + 0 * gamma * Q = the shaped rewards themselves:

  shape_state, shape_next (N,16)  uint8 codes: transitions of step_transitions.npz (real moves, invalid moves with state = next
                                  state, finished games), then constructed pairs: every max tile 2 .. 131072 with the max in (3,3),
                                  in (0,0), in both, in neither, with a new maximum and without; one tile; full boards of merge pairs
  shape_reward (N,)               float32: what torch.tensor(rewards, dtype=float32) made of the reward (negative and fractional ones)
  shape_out (N,)                  float32: the reference's shaped_rewards

Buffer. Scripted runs of the real buffer; run r is described by
  r<r>_capacity, r<r>_alpha, r<r>_kind (K,) 0 push / 1 sample / 2 update, r<r>_arg (K,) transitions pushed / batch size,
  r<r>_beta (K,)
and op k of it by
  r<r>_prio_<k>                   float32: the priorities in deque order after the op
  push:    the next r<r>_arg[k] rows of the pool (pool_state, pool_next, pool_action, pool_reward float32, pool_done)
  sample:  r<r>_u_<k> float64 (the uniforms np.random.choice drew: a twin RandomState at the same seed), r<r>_idx_<k>,
           r<r>_probs_<k> float32 (the p= handed to np.random.choice), r<r>_w_<k> float32, the sampled transitions
           r<r>_sstate_<k> / _snext_ / _saction_ / _sreward_ / _sdone_, and r<r>_perr_<k> / r<r>_werr_<k>: the largest absolute error
           of the reference's float32 probs / weights against the float64 evaluation of its formula on the same priorities
  update:  r<r>_uidx_<k>, r<r>_td_<k> float32: update_priorities(uidx, td + 1e-5) as train_step calls it (:1063-1064)

It asserts that cdf.searchsorted(u, 'right') on the recorded probs reproduces the recorded indices, that at most 1 % of each
call's draws lie within 2 ** -21 of a cdf entry (the draws a float32 re-evaluation of the probabilities may move), that
tests/per_ref.py reproduces everything, and that the file stays below 400 KB.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2:
    sys.exit(__doc__)
REF = sys.argv[1]
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)
import per_ref as R  # noqa: E402
with contextlib.redirect_stdout(io.StringIO()):
    import agents.hybrid as hyb  # noqa: E402

BATCH = 256


def tiles(codes):
    return R.tiles_f32(codes)


# ------------------------------------------------------------------------------------------------------------- shaping --
def constructed_pairs(rng):
    states, nexts = [], []
    for mc in range(1, 18):
        for corner in range(4):                      # bit 0: the max in (3,3); bit 1: the max in (0,0)
            for relation in range(3):                # previous max lower / equal / higher
                for fill in (0.2, 0.5, 1.0):
                    hi = max(mc - 1, 1)
                    nb = rng.integers(1, hi + 1, size=16).astype(np.uint8) if mc > 1 else np.zeros(16, np.uint8)
                    nb[rng.random(16) >= fill] = 0
                    nb[[0, 15]] = np.minimum(nb[[0, 15]], max(mc - 1, 0))
                    if corner & 1:
                        nb[15] = mc
                    if corner & 2:
                        nb[0] = mc
                    if corner == 0:
                        nb[rng.choice([1, 2, 5, 6, 9, 12, 3])] = mc
                    pb = np.minimum(rng.permutation(nb), max(mc - 1, 0)).astype(np.uint8)
                    if relation == 1:
                        pb[rng.integers(16)] = mc
                    elif relation == 2 and mc < 17:
                        pb[rng.integers(16)] = mc + 1
                    elif relation == 0 and pb.max() == mc:
                        pb[pb == mc] = 0
                    states.append(pb)
                    nexts.append(nb)
    for cell in (0, 5, 15):                          # one tile
        for code in (1, 2, 7, 17):
            nb = np.zeros(16, np.uint8)
            nb[cell] = code
            states.append(nb.copy())
            nexts.append(nb)
    states.append(np.zeros(16, np.uint8))            # the empty board: the loop's `if max_tile > 0` is false
    nexts.append(np.zeros(16, np.uint8))
    for k in range(40):                              # full boards with many merge pairs
        a, b = rng.integers(1, 17, size=2)
        nb = np.where((np.arange(16) // (4 if k & 1 else 2)) % 2 == 0, a, b).astype(np.uint8)
        if k % 4 >= 2:
            nb[:] = a
        states.append(rng.permutation(nb))
        nexts.append(nb)
    return np.array(states, np.uint8), np.array(nexts, np.uint8)


class StubBuffer:
    def __init__(self):
        self.batch = None

    def __len__(self):
        return BATCH

    def sample(self, batch_size, beta=0.4):
        assert batch_size == len(self.batch)
        return self.batch, list(range(batch_size)), np.ones(batch_size, np.float32)

    def update_priorities(self, indices, priorities):
        pass


def gen_shaping(tr):
    rng = np.random.default_rng(20482)
    invalid = np.flatnonzero(tr["valid"] == 0)[:300]
    done = np.flatnonzero(tr["done"] == 1)[:100]
    rest = rng.choice(len(tr["valid"]), 2200, replace=False)
    pick = np.unique(np.concatenate([invalid, done, rest]))
    pick = pick[np.isfinite(tr["reward"][pick])]
    st, nx = tr["board_in"][pick], tr["board_out"][pick]
    rw = tr["reward"][pick]
    cs, cn = constructed_pairs(rng)
    crw = np.round(rng.normal(0.0, 40.0, len(cs)), 3)
    crw[::7] = -np.abs(crw[::7]) - 0.1
    crw[::11] = rng.integers(0, 4096, len(crw[::11])) * 4.0
    st, nx, rw = np.concatenate([st, cs]), np.concatenate([nx, cn]), np.concatenate([rw, crw])
    pad = -len(st) % BATCH
    st, nx, rw = np.concatenate([st, st[:pad]]), np.concatenate([nx, nx[:pad]]), np.concatenate([rw, rw[:pad][::-1]])
    n = len(st)

    torch.manual_seed(0)
    model, target = torch.nn.Linear(16, 4), torch.nn.Linear(16, 4)
    stub = StubBuffer()
    with contextlib.redirect_stdout(io.StringIO()):
        agent = hyb.DQNAgent(hyb.Game2048Env(), model, target, stub, batch_size=BATCH)
    agent.device = torch.device("cpu")
    model.to("cpu")
    target.to("cpu")
    seen = []
    real_loss = hyb.nn.SmoothL1Loss

    def observed_loss(reduction="mean"):
        fn = real_loss(reduction=reduction)

        def call(current, wanted):
            seen.append(wanted.detach().numpy().copy())
            return fn(current, wanted)
        return call
    hyb.nn.SmoothL1Loss = observed_loss
    try:
        out = np.zeros(n, np.float32)
        rw32 = np.zeros(n, np.float32)
        for lo in range(0, n, BATCH):
            stub.batch = [(tiles(st[i]), 0, float(rw[i]), tiles(nx[i]), 1.0) for i in range(lo, lo + BATCH)]
            agent.train_step()
            assert len(seen) == lo // BATCH + 1 and seen[-1].dtype == np.float32
            out[lo:lo + BATCH] = seen[-1]
            rw32[lo:lo + BATCH] = torch.tensor([float(r) for r in rw[lo:lo + BATCH]], dtype=torch.float32).numpy()
    finally:
        hyb.nn.SmoothL1Loss = real_loss
    assert np.isfinite(out).all()
    mine = R.shaped_rewards(st, nx, rw32)
    bad = np.flatnonzero(mine != out)
    assert len(bad) == 0, ("tests/per_ref.py differs from the reference", bad[:10], mine[bad[:10]], out[bad[:10]])
    mx, pmx = nx.max(axis=1), st.max(axis=1)
    checks = {"invalid moves": (st == nx).all(axis=1).sum(), "max 64": (mx == 6).sum(), "max 128": (mx == 7).sum(),
              "max 131072": (mx == 17).sum(), "max in (3,3), above 64": ((nx[:, 15] == mx) & (mx > 6)).sum(),
              "max in (0,0) only, above 64": ((nx[:, 0] == mx) & (nx[:, 15] != mx) & (mx > 6)).sum(),
              "max in both": ((nx[:, 0] == mx) & (nx[:, 15] == mx)).sum(),
              "max in neither, above 64": ((nx[:, 0] != mx) & (nx[:, 15] != mx) & (mx > 6)).sum(),
              "new maximum": (mx > pmx).sum(), "no new maximum": (mx <= pmx).sum(), "one tile": ((nx > 0).sum(axis=1) == 1).sum(),
              "full": ((nx > 0).sum(axis=1) == 16).sum(), "negative reward": (rw32 < 0).sum(),
              "fractional reward": (rw32 != np.round(rw32)).sum()}
    print("shaping: %d triples; %s" % (n, ", ".join("%s %d" % kv for kv in checks.items())))
    assert n >= 3000 and all(v >= 3 for v in checks.values()), checks
    return dict(shape_state=st, shape_next=nx, shape_reward=rw32, shape_out=out)


# -------------------------------------------------------------------------------------------------------------- buffer --
PUSH, SAMPLE, UPDATE = 0, 1, 2


def run_script(r, capacity, alpha, ops, pool, cursor, rng, out):
    """ops: (PUSH, m) / (SAMPLE, batch, beta) / (UPDATE, how). Returns the pool cursor after the run."""
    buf = hyb.PrioritizedReplayBuffer(capacity, alpha=alpha)
    mine = R.Buffer(capacity, alpha)
    real_choice = np.random.choice
    last = {}
    kinds, args, betas = [], [], []
    for k, op in enumerate(ops):
        kinds.append(op[0])
        args.append(op[1] if op[0] != UPDATE else 0)
        betas.append(op[2] if op[0] == SAMPLE else 0.0)
        tag = "r%d_%%s_%d" % (r, k)
        if op[0] == PUSH:
            m = op[1]
            rows = slice(cursor, cursor + m)
            assert cursor + m <= len(pool["action"]), "the pool is too small"
            for i in range(cursor, cursor + m):
                buf.push(tiles(pool["state"][i]), int(pool["action"][i]), float(pool["reward"][i]), tiles(pool["next"][i]),
                         bool(pool["done"][i]))
            mine.push(pool["state"][rows], pool["action"][rows], pool["reward"][rows], pool["next"][rows], pool["done"][rows])
            cursor += m
        elif op[0] == SAMPLE:
            batch, beta = op[1], op[2]
            seed = 1000 * r + k
            seen = {}

            def choice(a, size=None, replace=True, p=None):
                seen["p"] = np.array(p, copy=True)
                return real_choice(a, size, replace, p)
            np.random.choice = choice
            try:
                np.random.seed(seed)
                samples, indices, weights = buf.sample(batch, beta=beta)
            finally:
                np.random.choice = real_choice
            u = np.random.RandomState(seed).random_sample(batch)
            probs = seen["p"]
            assert probs.dtype == np.float32 and weights.dtype == np.float32 and len(probs) == len(buf)
            cdf = R.cdf_of(probs)
            assert np.array_equal(R.search(cdf, u), indices), "the twin RandomState did not reproduce np.random.choice"
            near = R.near_cdf(cdf, u, 2.0 ** -21).mean()
            assert near <= 0.01, near
            prio = np.array(buf.priorities, dtype=np.float32)
            p64 = R.probs_f64(prio, alpha)
            w64 = R.weights_f64(p64, indices, len(buf), beta)
            mi, mp, mw = mine.sample(u, beta)
            assert np.array_equal(mi, indices) and np.array_equal(mp, probs) and np.array_equal(mw, weights)
            s, a, rw, nx, d = zip(*samples)
            codes = lambda t: np.where(np.array(t) > 0, np.log2(np.maximum(np.array(t), 1)), 0).astype(np.uint8)   # noqa: E731
            out.update({tag % "u": u, tag % "idx": np.asarray(indices, np.int64), tag % "probs": probs, tag % "w": weights,
                        tag % "perr": np.float64(np.abs(probs.astype(np.float64) - p64).max()),
                        tag % "werr": np.float64(np.abs(weights.astype(np.float64) - w64).max()),
                        tag % "sstate": codes(s), tag % "snext": codes(nx), tag % "saction": np.array(a, np.uint8),
                        tag % "sreward": np.array(rw, np.float32), tag % "sdone": np.array(d, np.uint8)})
            assert np.array_equal(out[tag % "sstate"], mine.states[indices]) and np.array_equal(out[tag % "sreward"], mine.rewards[indices])
            last = dict(indices=np.asarray(indices, np.int64), near=near, dup=batch - len(np.unique(indices)))
            print("  run %d op %d: sample %d of %d, beta %.1f: %d duplicates, %.2f %% of the draws near a cdf entry, reference error "
                  "probs %.3g weights %.3g" % (r, k, batch, len(buf), beta, last["dup"], 100 * near, out[tag % "perr"], out[tag % "werr"]))
        else:
            how = op[1]
            if how == "sampled":                     # what train_step does, with zero, tiny and negative td errors among them
                uidx = last["indices"].copy()
                assert last["dup"] > 0
                td = rng.exponential(1.0, len(uidx)).astype(np.float32)
                td[::9] = 0.0
                td[1::9] = np.float32(3e-6)
                td[2::9] = np.float32(-1e-3)
                td[3::9] = np.float32(1e-7)
                uidx[-3:] = [len(buf), len(buf) + 7, capacity + 1]            # beyond the live entries: ignored (:761)
            else:                                    # "spike": one priority 10 ** 4 times the rest
                uidx = np.arange(len(buf), dtype=np.int64)
                td = np.full(len(buf), 1.0, np.float32)
                td[len(buf) // 3] = np.float32(1e4)
            with torch.no_grad():
                priorities = (torch.from_numpy(td) + 1e-5).detach().cpu().numpy()        # :1063
            buf.update_priorities(uidx, priorities)                                     # :1064
            mine.update_priorities(uidx, td)
            out.update({tag % "uidx": uidx, tag % "td": td})
        prio = np.array(buf.priorities, dtype=np.float32)
        assert np.array_equal(prio, mine.priorities), ("tests/per_ref.py differs from the reference", r, k)
        out[tag % "prio"] = prio
    out.update({"r%d_capacity" % r: np.int64(capacity), "r%d_alpha" % r: np.float64(alpha), "r%d_kind" % r: np.array(kinds, np.uint8),
                "r%d_arg" % r: np.array(args, np.int64), "r%d_beta" % r: np.array(betas, np.float64)})
    return cursor


RUNS = [
    (1000, 0.6, [(PUSH, 700), (SAMPLE, 256, 0.4), (UPDATE, "sampled"), (PUSH, 600), (SAMPLE, 256, 0.7), (UPDATE, "sampled"),
                 (PUSH, 250), (SAMPLE, 256, 1.0)]),
    (1000, 0.85, [(PUSH, 700), (SAMPLE, 128, 0.4), (UPDATE, "sampled"), (PUSH, 600), (SAMPLE, 128, 0.7), (UPDATE, "sampled"),
                  (PUSH, 250), (SAMPLE, 128, 1.0)]),
    (65, 0.6, [(PUSH, 50), (SAMPLE, 32, 0.4), (UPDATE, "sampled"), (PUSH, 40), (SAMPLE, 32, 0.7), (UPDATE, "sampled"), (PUSH, 65),
               (SAMPLE, 65, 1.0)]),
    (1000, 0.6, [(PUSH, 700), (UPDATE, "spike"), (SAMPLE, 256, 0.4), (PUSH, 100), (SAMPLE, 256, 0.7)]),
]


def main():
    torch.set_num_threads(1)
    tr = np.load(os.path.join(HERE, "step_transitions.npz"))
    out = gen_shaping(tr)
    rng = np.random.default_rng(20483)
    rows = rng.permutation(np.flatnonzero(np.isfinite(tr["reward"])))[:4100]
    pool = dict(state=tr["board_in"][rows], next=tr["board_out"][rows], action=tr["action"][rows],
                reward=tr["reward"][rows].astype(np.float32), done=tr["done"][rows])
    out.update({"pool_" + k: v for k, v in pool.items()})
    cursor = 0
    for r, (capacity, alpha, ops) in enumerate(RUNS):
        cursor = run_script(r, capacity, alpha, ops, pool, cursor, rng, out)
    out["runs"] = np.int64(len(RUNS))
    assert cursor <= len(rows)
    path = os.path.join(HERE, "per.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes, %d pool rows used" % (path, os.path.getsize(path), cursor))
    assert os.path.getsize(path) <= 400_000


if __name__ == "__main__":
    main()
