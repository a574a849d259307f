#!/usr/bin/env python3
"""Golden vectors of the hybrid agent's Q-network: runs the REFERENCE's own class on fixed weights and records outputs.

Usage (needs a checkout of the reference; the tests never read it, only the file this writes):

    python tests/golden/gen_qnet_golden.py <reference checkout>

The reference ships no trained hybrid model, so the pin is its class, agents/hybrid.py HybridDQN() (2 layers, dim_feedforward
2048), imported read-only via sys.path (nothing is copied), on the weights of tests/qnet_weights.py: 1,326,180 parameters
derived from a few integers, which are therefore not stored. The class is run in .eval() with ONE board per call, the only way
the reference calls it (a batch would be one sequence of tokens that attend to each other); the equivalent form with the
encoder input reshaped to (1, B, 128) is checked against it. Inputs are the boards of policy.npz as the env's get_state():
2 ** code, 0 for empty. It writes qnet.npz in this directory (data only):

  recipe_names, recipe_values   the integers of qnet_weights.RECIPE
  dim_ff, n_layers              2048, 2
  tensor_names, tensor_crc32    the state dict's names in order and the CRC-32 of each tensor's float32 bytes
  q_f64                         the class in .double(): the truth
  q_f32                         the same class in float32 (what stock torch gives on CPU)
  q_bf16w                       the class in float64 with every parameter rounded to bfloat16 first: the error the weights alone
                                cost
  actions_f64                   the exploit action of DQNAgent.select_action (hybrid.py:947-953) on q_f64, the valid-move mask
                                from the project's CPU oracle

The boards themselves are those of policy.npz and are not stored again. It asserts the conditions that make the fixture pin
something: at least two actions are the masked argmax on >= 10 % of the boards each, and the share of boards whose top-two
valid-move gap in q_f64 is within twice the tests' Q bound stays within the tests' caps (f32: bound 8 x |q_f32 - q_f64|, cap
1 %; bf16: bound 4 x |q_bf16w - q_f64|, cap 20 %).
"""
import os
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
from agents.hybrid import HybridDQN  # noqa: E402
from oracle import oracle as O  # noqa: E402

F32_FACTOR, BF16_FACTOR, F32_CAP, BF16_CAP = 8.0, 4.0, 0.01, 0.20


def check_conditions(out, valid):
    counts = np.bincount(out["actions_f64"], minlength=4)
    assert (counts >= 0.1 * len(valid)).sum() >= 2, counts
    gap = qw.top_two_gap(out["q_f64"], valid)
    shares = []
    for key, factor, cap in (("q_f32", F32_FACTOR, F32_CAP), ("q_bf16w", BF16_FACTOR, BF16_CAP)):
        bound = factor * np.abs(out[key] - out["q_f64"]).max()
        share = float((gap <= 2 * bound).mean())
        assert share <= cap, (key, share, cap)
        shares.append(share)
    return counts, shares


def main():
    torch.manual_seed(0)
    shapes = [(k, tuple(v.shape)) for k, v in HybridDQN().state_dict().items()]
    assert shapes == qw.reference_shapes(), "the reference's state dict is not the one qnet_weights.reference_shapes lists"
    sd = qw.state_dict(shapes)
    assert sum(v.size for v in sd.values()) == qw.N_PARAMETERS
    codes = np.load(os.path.join(HERE, "policy.npz"))["boards"]
    tiles = np.where(codes > 0, 2.0 ** codes.astype(np.float64), 0.0)
    out = {"recipe_names": np.array(sorted(qw.RECIPE)), "recipe_values": np.array([qw.RECIPE[k] for k in sorted(qw.RECIPE)], np.int64),
           "dim_ff": np.int64(2048), "n_layers": np.int64(2), "tensor_names": np.array([k for k, _ in shapes]),
           "tensor_crc32": np.array([qw.checksum(sd[k]) for k, _ in shapes], np.uint32)}

    def run(dtype, rounded):
        m = HybridDQN().eval().to(dtype)
        t = {k: torch.from_numpy(v) for k, v in sd.items()}
        if rounded:
            t = {k: v.float().bfloat16().double() for k, v in t.items()}
        m.load_state_dict({k: v.to(dtype) for k, v in t.items()})
        x = torch.from_numpy(tiles).to(dtype)
        with torch.no_grad():
            q = torch.cat([m(x[i:i + 1]) for i in range(len(x))])
            if dtype == torch.float64:         # the (1, B, 128) form is the same function
                h = m.embedding(m.cnn(x.view(-1, 1, 4, 4)).view(len(x), -1))
                alt = m.fc(m.transformer(h.unsqueeze(0)).squeeze(0))
                assert (alt - q).abs().max() <= 1e-12, (alt - q).abs().max()
                assert (m(x[:512]) - q[:512]).abs().max() > 1e-3, "a batch call no longer mixes its boards"
        return q.numpy()

    out["q_f64"] = run(torch.float64, False)
    out["q_f32"] = run(torch.float32, False)
    out["q_bf16w"] = run(torch.float64, True)
    valid = qw.mask_bits(O.valid_moves_batch(codes))
    out["actions_f64"] = qw.masked_argmax(out["q_f64"], valid)
    qmax = np.abs(out["q_f64"]).max()
    print("max|Q| %.4g; f32 vs f64 %.3g, bf16 weights vs f64 %.3g of max|Q|; argmax counts %s" % (
        qmax, np.abs(out["q_f32"] - out["q_f64"]).max() / qmax, np.abs(out["q_bf16w"] - out["q_f64"]).max() / qmax,
        np.bincount(out["actions_f64"], minlength=4).tolist()))
    counts, shares = check_conditions(out, valid)
    path = os.path.join(HERE, "qnet.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes; boards within twice the bound of a tie: f32 %.2f %%, bf16 %.2f %%" % (
        path, os.path.getsize(path), 100 * shares[0], 100 * shares[1]))
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "policy.npz")), "qnet.npz must not exceed policy.npz"


if __name__ == "__main__":
    main()
