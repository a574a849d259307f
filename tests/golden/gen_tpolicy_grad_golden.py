#!/usr/bin/env python3
"""Golden gradients of the transformer policy's PPO loss: runs the REFERENCE's own TransformerModel through the lines of
PPOAgent.update()'s loss (agents/ppo_agent.py:378-400, up to backward()) on its two heads and records inputs -> losses and gradients.

Usage (needs a checkout of the reference; the tests never read it, only the file this writes):

    python tests/golden/gen_tpolicy_grad_golden.py <reference checkout>

It imports models/transformer.py of the reference read-only via sys.path (nothing is copied), gives TransformerModel().eval() the
weights of tests/tpolicy_weights.py (derived from a few integers, so not stored) and writes tpolicy_grad.npz here (data only). This
docstring is the file's only description: the table in README.md here has no row for it.

  start                         int64: the 32 rows are boards[start : start + 32] of policy.npz
  noise                         float64: the scale of the noise in old_log_probs
  boards                        uint8 (32, 16)
  actions (int64), old_log_probs, advantages, returns (float32)    the inputs by the recipe of tests/tpolicy_grad_ref.py
  losses_f64                    loss, actor_loss, value_loss, entropy of the class in .double()
  probs_f64, value_f64          its forward
  tensor_names                  the state dict's names in order
  grad.<name>                   float64: the gradient, flattened; tensors of at most 4,096 elements in full, larger ones at every
                                97th flat index (tests/tpolicy_grad_ref.py golden_positions)
  gmax                          float64 per tensor: max|g| over the WHOLE tensor
  yardstick_f32                 the worst max|g32 - g64| / max|g64| per tensor of the same class in float32 on the same inputs

The lines :378-400 themselves are tests/tpolicy_grad_ref.py's stock_loss_grad, written against torch's modules; here it is handed
the reference's class. It asserts what makes the fixture pin something: the clipped branch is the minimum on 10 .. 90 % of the
rows, advantages of both signs, every tensor's max|g| > 0, a float32 yardstick > 0. If the band is missed, change the noise
scale, not the band.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2:
    sys.exit(__doc__)
REF = sys.argv[1]
TESTS = os.path.dirname(HERE)
for p in (TESTS, os.path.dirname(TESTS), REF):
    sys.path.insert(0, p)
from models.transformer import TransformerModel  # noqa: E402
import tpolicy_grad_ref as R  # noqa: E402
import tpolicy_weights as tw  # noqa: E402

START, NOISE, SEED = 0, 0.5, 0


def main():
    boards = np.ascontiguousarray(np.load(os.path.join(HERE, "policy.npz"))["boards"][START:START + R.GOLDEN_ROWS])
    shapes = tw.reference_shapes()
    sd = tw.state_dict(shapes)
    models = {}
    for dtype in (torch.float64, torch.float32):
        m = TransformerModel().eval().to(dtype)
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == shapes
        m.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in sd.items()})
        models[dtype] = m
    actions, old, adv, ret = R.recipe(models[torch.float64], boards, SEED, NOISE)
    want = R.stock_loss_grad(models[torch.float64], boards, actions, old, adv, ret)
    f32 = R.stock_loss_grad(models[torch.float32], boards, actions, old, adv, ret)
    share = float(want["clipped"].mean())
    gmax = np.array([np.abs(g).max() for g in want["grads"]])
    yard = float(R.ratios(f32["grads"], want["grads"]).max())
    assert R.BAND[0] <= share <= R.BAND[1], "clipped share %.2f: change NOISE, not the band" % share
    assert (adv > 0).any() and (adv < 0).any()
    assert (gmax > 0).all(), "a gradient tensor is zero"
    assert yard > 0
    names = [k for k, _ in shapes]
    assert len(names) == len(want["grads"])
    out = dict(start=np.int64(START), noise=np.float64(NOISE), boards=boards, actions=actions, old_log_probs=old, advantages=adv, returns=ret,
               losses_f64=want["losses"], probs_f64=want["probs"], value_f64=want["value"], tensor_names=np.array(names), gmax=gmax,
               yardstick_f32=np.float64(yard))
    for k, g in zip(names, want["grads"]):
        out["grad." + k] = g[R.golden_positions(g.size)]
    path = os.path.join(HERE, "tpolicy_grad.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes; clipped share %.2f, losses %s, max|g| %.3g .. %.3g, float32 yardstick %.3g"
          % (path, os.path.getsize(path), share, want["losses"].round(4).tolist(), gmax.min(), gmax.max(), yard))
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "ppo_update.npz")), "tpolicy_grad.npz must not exceed ppo_update.npz"


if __name__ == "__main__":
    main()
