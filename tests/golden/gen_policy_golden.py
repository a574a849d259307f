#!/usr/bin/env python3
"""Golden vectors of the reference's PPO actor / critic: runs the REFERENCE's own networks and records inputs -> outputs.

Usage (needs a checkout of the reference; the tests never read it, only the file this writes):

    python tests/golden/gen_policy_golden.py <reference checkout>

It imports agents/ppo_agent.py of the reference read-only via sys.path (nothing is copied), loads the trained
checkpoints/final_model.pth it ships, and writes policy.npz in this directory (data only):

  actor.<name>, critic.<name>   the two state dicts as float32 arrays (num_batches_tracked dropped)
  boards                        uint8 (2048, 16) log2 codes: board_in of the first 1,024 rows of step_transitions.npz and
                                1,024 states of the three long width-20 / depth-30 games of games.npz (every 2nd state, the first 1,024)
  probs_batched, values_batched the networks in eval mode on CPU, ONE call on all 2,048 normalized boards (BatchNorm active)
  probs_single, values_single   one call per board (a (16,) input, BatchNorm skipped) for the first 128 boards

The observations are the reference's own PPOAgent.normalize_state of the tile values.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path.insert(0, REF)
from agents.ppo_agent import ActorNetwork, CriticNetwork, PPOAgent  # noqa: E402

N_SINGLE = 128


def boards():
    st = np.load(os.path.join(HERE, "step_transitions.npz"))["board_in"][:1024]
    g = np.load(os.path.join(HERE, "games.npz"))
    games = np.concatenate([g["g%d_boards" % i] for i in (12, 13, 14)])[::2][:1024]
    return np.ascontiguousarray(np.concatenate([st, games]).astype(np.uint8))


def main():
    torch.manual_seed(0)
    ck = torch.load(os.path.join(REF, "checkpoints", "final_model.pth"), map_location="cpu", weights_only=False)
    actor, critic = ActorNetwork(), CriticNetwork()
    actor.load_state_dict(ck["actor_state_dict"])
    critic.load_state_dict(ck["critic_state_dict"])
    actor.eval()
    critic.eval()
    b = boards()
    tiles = np.where(b > 0, 1 << b.astype(np.int64), 0)
    agent = PPOAgent.__new__(PPOAgent)          # normalize_state uses no instance state
    x = np.stack([agent.normalize_state(t) for t in tiles]).astype(np.float32)
    assert np.array_equal(x, b.astype(np.float32) / np.float32(15.0))
    out = {"boards": b}
    for prefix, sd in (("actor.", ck["actor_state_dict"]), ("critic.", ck["critic_state_dict"])):
        for k, v in sd.items():
            if k.endswith("num_batches_tracked"):
                continue
            out[prefix + k] = v.detach().float().numpy()
    with torch.no_grad():
        xt = torch.from_numpy(x)
        out["probs_batched"] = actor(xt).numpy()
        out["values_batched"] = critic(xt).numpy()
        out["probs_single"] = np.stack([actor(xt[i]).numpy() for i in range(N_SINGLE)])
        out["values_single"] = np.stack([critic(xt[i]).numpy() for i in range(N_SINGLE)])
    path = os.path.join(HERE, "policy.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes, %d boards, max |value| %.1f" % (path, os.path.getsize(path), len(b), np.abs(out["values_batched"]).max()))


if __name__ == "__main__":
    main()
