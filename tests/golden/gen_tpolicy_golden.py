#!/usr/bin/env python3
"""Golden vectors of the reference's transformer policy: runs the REFERENCE's own class on fixed weights and records outputs.

Usage (needs a checkout of the reference; the tests never read it, only the file this writes):

    python tests/golden/gen_tpolicy_golden.py <reference checkout>

The reference ships no trained transformer, so the pin is its class, models/transformer.py TransformerModel() with its
defaults (2 layers, dim_feedforward 2048), imported read-only via sys.path (nothing is copied), on the weights of
tests/tpolicy_weights.py: 702,213 parameters derived from a few integers, which are therefore not stored. It writes tpolicy.npz
in this directory (data only):

  recipe_names, recipe_values   the integers of tpolicy_weights.RECIPE
  dim_ff, n_layers              2048, 2
  tensor_names, tensor_crc32    the state dict's names in order and the CRC-32 of each tensor's float32 bytes
  boards                        uint8 (2048, 16): the boards of policy.npz
  probs_f64, value_f64          the class in .double() on x = boards / 15: the truth
  probs_f32, value_f32          the same class in float32 (what stock torch gives on CPU)
  probs_bf16w, value_bf16w      the class in float64 with every parameter rounded to bfloat16 first: the error the weights
                                alone cost

It asserts the conditions that make the fixture pin something: over the 2,048 boards the largest probability ranges from
below 0.5 to above 0.9, and at least two actions are the argmax on >= 10 % of the boards each.
"""
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
import tpolicy_weights as tw  # noqa: E402
from models.transformer import TransformerModel  # noqa: E402


def check_conditions(probs):
    top = probs.max(1)
    counts = np.bincount(probs.argmax(1), minlength=4)
    assert top.min() < 0.5 and top.max() > 0.9, (top.min(), top.max())
    assert (counts >= 0.1 * len(probs)).sum() >= 2, counts
    return top, counts


def main():
    torch.manual_seed(0)
    model = TransformerModel().eval()
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    assert shapes == tw.reference_shapes(), "the reference's state dict is not the one tpolicy_weights.reference_shapes lists"
    sd = tw.state_dict(shapes)
    b = np.load(os.path.join(HERE, "policy.npz"))["boards"]
    out = {"recipe_names": np.array(sorted(tw.RECIPE)), "recipe_values": np.array([tw.RECIPE[k] for k in sorted(tw.RECIPE)], np.int64),
           "dim_ff": np.int64(2048), "n_layers": np.int64(2), "tensor_names": np.array([k for k, _ in shapes]),
           "tensor_crc32": np.array([tw.checksum(sd[k]) for k, _ in shapes], np.uint32), "boards": b}

    def run(dtype, rounded):
        m = TransformerModel().eval().to(dtype)
        t = {k: torch.from_numpy(v) for k, v in sd.items()}
        if rounded:
            t = {k: v.float().bfloat16().double() for k, v in t.items()}
        m.load_state_dict({k: v.to(dtype) for k, v in t.items()})
        with torch.no_grad():
            p, v = m(torch.from_numpy(b).to(dtype) / 15)
        return p.numpy(), v.numpy()

    out["probs_f64"], out["value_f64"] = run(torch.float64, False)
    out["probs_f32"], out["value_f32"] = run(torch.float32, False)
    out["probs_bf16w"], out["value_bf16w"] = run(torch.float64, True)
    top, counts = check_conditions(out["probs_f64"])
    path = os.path.join(HERE, "tpolicy.npz")
    np.savez_compressed(path, **out)
    vmax = np.abs(out["value_f64"]).max()
    print("%s: %d bytes; largest probability %.3f .. %.3f, argmax counts %s, values %.2f .. %.2f" % (
        path, os.path.getsize(path), top.min(), top.max(), counts.tolist(), out["value_f64"].min(), out["value_f64"].max()))
    print("f32 vs f64: probs %.3g, values %.3g of max|v|; bf16 weights vs f64: probs max %.3g mean %.3g, values %.3g of max|v|" % (
        np.abs(out["probs_f32"] - out["probs_f64"]).max(), np.abs(out["value_f32"] - out["value_f64"]).max() / vmax,
        np.abs(out["probs_bf16w"] - out["probs_f64"]).max(), np.abs(out["probs_bf16w"] - out["probs_f64"]).mean(),
        np.abs(out["value_bf16w"] - out["value_f64"]).max() / vmax))
    assert os.path.getsize(path) <= 405302, "tpolicy.npz must not exceed policy.npz"


if __name__ == "__main__":
    main()
