#!/usr/bin/env python3
"""Golden gradients of the reference's PPO update: runs the REFERENCE's own ActorNetwork / CriticNetwork through the epoch body of
PPOAgent.update() (agents/ppo_agent.py:378-400, up to backward()) and records inputs -> losses and gradients.

Usage (needs a checkout of the reference; the tests never read it, only the file this writes):

    python tests/golden/gen_ppo_update_golden.py <reference checkout>

It imports agents/ppo_agent.py of the reference read-only via sys.path (nothing is copied), gives the two classes the trained
weights and running statistics of policy.npz in this directory, sets dropout p = 0, puts them in training mode and in float64,
and writes ppo_update.npz here (data only, float32 unless noted). This docstring is the file's only description: the table in
README.md here has no row for it.

  start                         int64: the 32 rows are boards[start : start + 32] of policy.npz, the first window of 32 in which
                                every ReLU input keeps the margin of tests/ppo_update_ref.py
  states                        (32, 16) the observations codes / 15
  actions (int64), old_log_probs, advantages, returns    the inputs by the recipe of tests/ppo_update_ref.py
  losses                        loss, actor_loss, value_loss, entropy
  probs, values                 the training-mode forwards
  grad.<k>                      the 24 gradients, actor then critic, each in named_parameters() order, flattened
  running.<k>                   the 8 running statistics after the one forward

The lines :378-400 themselves are tests/ppo_update_ref.py's stock_update, written against torch's modules; here it is handed the
reference's classes.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
TESTS = os.path.dirname(HERE)
for p in (TESTS, os.path.dirname(TESTS), REF):
    sys.path.insert(0, p)
from agents.ppo_agent import ActorNetwork, CriticNetwork  # noqa: E402
import ppo_update_ref as R  # noqa: E402

ROWS = 32


def main():
    g = np.load(os.path.join(HERE, "policy.npz"))
    nets = ActorNetwork(), CriticNetwork()
    for net, prefix in zip(nets, ("actor.", "critic.")):
        sd = {k[len(prefix):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)}
        missing = net.load_state_dict(sd, strict=False)
        assert all(k.endswith("num_batches_tracked") for k in missing.missing_keys) and not missing.unexpected_keys
        net.dropout.p = 0.0
        net.double().train()
    boards = g["boards"].astype(np.float32) / np.float32(15.0)
    for start in range(0, len(boards) - ROWS + 1):
        x = np.ascontiguousarray(boards[start:start + ROWS])
        if R.relu_margin(nets, torch.from_numpy(x).double()) >= R.RELU_MARGIN:
            break
    else:
        raise SystemExit("no window keeps the ReLU margin")
    actions, old, adv, ret = R.recipe(nets, x)
    res = R.stock_update(nets, x, actions, old, adv, ret)
    out = {"start": np.int64(start), "states": x, "actions": actions, "old_log_probs": old, "advantages": adv, "returns": ret,
           "losses": res["losses"].astype(np.float32), "probs": res["probs"].astype(np.float32), "values": res["values"].astype(np.float32)}
    for k, t in enumerate(res["grads"]):
        out["grad.%02d" % k] = t.astype(np.float32)
    for k, t in enumerate(res["running"]):
        out["running.%d" % k] = t.astype(np.float32)
    path = os.path.join(HERE, "ppo_update.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes (policy.npz: %d), start %d, probs %.4g .. %.4g, losses %s" % (
        path, os.path.getsize(path), os.path.getsize(os.path.join(HERE, "policy.npz")), start, res["probs"].min(), res["probs"].max(), res["losses"]))


if __name__ == "__main__":
    main()
