#!/usr/bin/env python3
"""Golden vectors of the hybrid Q-network's loss and gradient pass: runs the REFERENCE's own class through the lines of
DQNAgent.train_step that need gradients.

Usage (needs a checkout of the reference; the tests never read it, only the file this writes):

    python tests/golden/gen_qnet_grad_golden.py <reference checkout>

The class is imported read-only via sys.path (nothing is copied), in .eval() (the reference's live dropout has no counterpart in
this library), on the online weights of tests/qnet_weights.py (seed 1, the recipe of qnet.npz). agents/hybrid.py:1038 and
:1049-1055 are executed as they are written there (model(states).gather(..), nn.SmoothL1Loss(reduction='none'), (weights *
td_errors).mean(), zero_grad, backward) in float64 and in float32, on three cases:

  early_17, early_256    boards with codes 0..3 (tiles <= 8): random_boards(256, 5) % 4 of tests/test_policy_host.py, stored
  full_256               the first 256 boards of policy.npz (tiles up to 131,072), not stored again

with, i the row index, actions = (5 i + 1) mod 4, weights = 0.25 + ((13 i) mod 16) / 16 and targets = float32(q64[i, a_i] +
((37 i + 11) mod 101 - 50) / 25). It writes qnet_grad.npz in this directory (data only):

  cases, tensor_names, upstream (1 where the tensor lies upstream of layer 0's softmax: cnn.*, embedding.*, layer 0's in_proj_*)
  early_boards uint8 [256][16]
  <case>_targets float32, <case>_loss_f64 / _f32, <case>_td_f64 / _f32, <case>_q_f64
  <case>_gmax_f64 [tensors]         max|g| of every tensor in float64
  <case>_norm_f64 / _f32 [tensors]  every tensor's gradient 2-norm
  <case>_err_f32 [tensors]          max|g32 - g64| / max|g64| over the WHOLE tensor
  positions [tensors][64]           hashed flat positions (mod the tensor's size), the same for every case
  <case>_g_f64 / _g_f32 [tensors][64]   the gradient entries at those positions

It asserts what makes the fixture a pin: both Huber branches hold >= 25 % of the rows and every action >= 10 % at n >= 17; on the
early-board cases stock float32 stays within 1e-5 x max|g| of float64 for every tensor. On full_256 float32 is NOT a fair
yardstick upstream of layer 0's softmax (logits up to 1e9, a nearly one-hot softmax): the error is recorded, not bounded.
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2:
    sys.exit(__doc__)
REF = sys.argv[1]
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)
import qnet_weights as qw  # noqa: E402
from test_policy_host import random_boards  # noqa: E402
from agents.hybrid import HybridDQN  # noqa: E402

SAMPLES = 64
UPSTREAM = ("cnn.", "embedding.", "transformer.layers.0.self_attn.in_proj_")


def recipe(n):
    i = np.arange(n, dtype=np.int64)
    return (5 * i + 1) % 4, ((37 * i + 11) % 101 - 50) / 25.0, (0.25 + ((13 * i) % 16) / 16.0).astype(np.float32)


def positions(t, numel):
    mask = (1 << 64) - 1
    return np.array([(((k * 0x9E3779B97F4A7C15 + t * 0xBF58476D1CE4E5B9) & mask) >> 17) % numel for k in range(SAMPLES)], np.int64)


def build(sd, dtype):
    m = HybridDQN().eval().to(dtype)
    m.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in sd.items()})
    return m


def train_lines(model, states, actions, target_q_values, weights):
    """agents/hybrid.py:1038 and :1049-1055, as written there (the optimizer's zero_grad is the module's)."""
    current_q_values = model(states).gather(1, actions.unsqueeze(1)).squeeze(1)
    loss_fn = nn.SmoothL1Loss(reduction='none')
    td_errors = loss_fn(current_q_values, target_q_values)
    weighted_loss = (weights * td_errors).mean()
    model.zero_grad()
    weighted_loss.backward()
    return weighted_loss.detach(), td_errors.detach()


def main():
    torch.manual_seed(0)
    shapes = [(k, tuple(v.shape)) for k, v in HybridDQN().state_dict().items()]
    assert shapes == qw.reference_shapes()
    sd = qw.state_dict(shapes)
    m64, m32 = build(sd, torch.float64), build(sd, torch.float32)
    names = [k for k, _ in m64.named_parameters()]
    assert names == [k for k, _ in shapes]
    early = (random_boards(256, 5) % 4).astype(np.uint8)
    full = np.load(os.path.join(HERE, "policy.npz"))["boards"][:256]
    pos = np.stack([positions(t, p.numel()) for t, p in enumerate(m64.parameters())])
    out = {"cases": np.array(["early_17", "early_256", "full_256"]), "tensor_names": np.array(names),
           "upstream": np.array([int(k.startswith(UPSTREAM)) for k in names], np.int64), "early_boards": early, "positions": pos}
    for case, codes in (("early_17", early[:17]), ("early_256", early), ("full_256", full)):
        n = len(codes)
        tiles = np.where(codes > 0, 2.0 ** codes.astype(np.float64), 0.0)
        a, offset, w = recipe(n)
        x64 = torch.from_numpy(tiles)
        with torch.no_grad():
            q64 = m64(x64).numpy()
        targets = (q64[np.arange(n), a] + offset).astype(np.float32)
        ta, tt, tw_ = torch.from_numpy(a), torch.from_numpy(targets), torch.from_numpy(w)
        loss64, td64 = train_lines(m64, x64, ta, tt.double(), tw_.double())
        loss32, td32 = train_lines(m32, x64.float(), ta, tt, tw_)
        d = q64[np.arange(n), a] - targets.astype(np.float64)
        quad = float((np.abs(d) < 1).mean())
        counts = np.bincount(a, minlength=4)
        print("%s: loss %.6g, quadratic branch %.1f %%, actions %s" % (case, float(loss64), 100 * quad, counts.tolist()))
        assert 0.25 <= quad <= 0.75 and counts.min() >= 0.1 * n
        g64 = [p.grad.numpy().reshape(-1) for p in m64.parameters()]
        g32 = [p.grad.numpy().reshape(-1).astype(np.float64) for p in m32.parameters()]
        gmax = np.array([np.abs(g).max() for g in g64])
        err = np.array([np.abs(b - g).max() for g, b in zip(g64, g32)]) / gmax
        up = out["upstream"].astype(bool)
        print("  float32 autograd vs float64, worst max|g32 - g64| / max|g64|: upstream of the layer-0 softmax %.3g, all other %.3g"
              % (err[up].max(), err[~up].max()))
        assert gmax.min() > 0
        if case.startswith("early"):
            assert err.max() <= 1e-5, err.max()
        out.update({case + "_targets": targets, case + "_loss_f64": np.float64(loss64), case + "_loss_f32": np.float32(loss32),
                    case + "_td_f64": td64.numpy(), case + "_td_f32": td32.numpy(), case + "_q_f64": q64, case + "_gmax_f64": gmax,
                    case + "_norm_f64": np.array([np.linalg.norm(g) for g in g64]), case + "_norm_f32": np.array([np.linalg.norm(g) for g in g32]),
                    case + "_err_f32": err, case + "_g_f64": np.stack([g[p] for g, p in zip(g64, pos)]),
                    case + "_g_f32": np.stack([g[p] for g, p in zip(g32, pos)]).astype(np.float32)})
    path = os.path.join(HERE, "qnet_grad.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
