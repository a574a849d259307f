#!/usr/bin/env python3
"""Golden vectors of the hybrid Q-network's BATCH call and of train_step's Double-DQN targets: runs the REFERENCE's own class.

Usage (needs a checkout of the reference; the tests never read it, only the file this writes):

    python tests/golden/gen_qnet_batch_golden.py <reference checkout>

DQNAgent.train_step (agents/hybrid.py:1038-1046) calls HybridDQN on a whole batch. The encoder layer is not batch_first and is
fed x.unsqueeze(1), so the B boards are ONE sequence of B tokens that attend to each other: a different function from the
per-board rows of qnet.npz. The class is imported read-only via sys.path (nothing is copied), in .eval(), on the weights of
tests/qnet_weights.py: the online network at seed 1 (the recipe of qnet.npz), the target network at the first seed >= 2 for
which the conditions below hold. The boards are the first B of policy.npz, B in SIZES, as the env's get_state() (2 ** code, 0
for empty); they are not stored again. It writes qnet_batch.npz in this directory (data only):

  sizes, target_seed, gamma
  shaped, dones                     float32 [max B], derived from the row index with integer arithmetic; dones mixed 0 / 1
  online_q_f64_<B>, target_q_f64_<B>    the literal batch call m(x[:B]) of the class in .double(): the truth
  online_q_f32_<B>, target_q_f32_<B>    the same call in float32 on the CPU (what stock torch gives; the tests' f32 yardstick)
  actions_f64_<B>                   argmax(1) of online_q_f64_<B> (unmasked, as :1042)
  targets_f64_<B>                   shaped + (1 - dones) * gamma * target_q_f64_<B>[i, actions_f64_<B>[i]] in float64

It asserts what makes the fixture a pin:
  (a) for both networks the batch call differs from the per-board rows by more than 0.1 x max|Q| at B >= 17;
  (b) conditioning: with every attention logit of the f64 network multiplied by 1 + 8 * 2**-24 * r, r uniform in [-1, 1], three
      seeds, Q moves by at most a quarter of the tests' f32 bound 8 x max|q_f32 - q_f64| (the first layer's logits reach 1e9 and
      its softmax is nearly one-hot; near-tied keys are near-identical boards with near-identical values, which is why this holds);
      and stock float32 itself stays within 1e-5 x max|Q| of the truth (the condition qnet.npz meets too): a case in which float32
      flips a near-tied key pins no f32 kernel (target seed 2 does at B = 300: 1.2e-3);
  (c) the share of boards whose top-two gap over all four online Q is within twice that bound is at most 1 %;
  (d) at B = 256 at least two actions are the online argmax on >= 10 % of the boards each.
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
import qnet_weights as qw  # noqa: E402
from agents.hybrid import HybridDQN  # noqa: E402

SIZES = (1, 17, 256, 300)
GAMMA, F32_FACTOR, TIE_CAP, NOISE = 0.99, 8.0, 0.01, 8 * 2.0 ** -24


def build(sd, dtype):
    m = HybridDQN().eval().to(dtype)
    m.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in sd.items()})
    return m


def spelled_out(m, x, noise=0.0, seed=0):
    """The module's batch call with the attention written out, the logits multiplied by 1 + noise * r."""
    gen = torch.Generator().manual_seed(seed)
    n = len(x)
    h = m.embedding(m.cnn(x.view(-1, 1, 4, 4)).view(n, -1))
    for lay in m.transformer.layers:
        a = lay.self_attn
        q, k, v = (h @ a.in_proj_weight.T + a.in_proj_bias).split(128, 1)
        s = torch.einsum("ihd,jhd->hij", q.view(n, 8, 16), k.view(n, 8, 16)) / 4.0
        if noise:
            s = s * (1 + noise * (2 * torch.rand(s.shape, generator=gen, dtype=torch.float64) - 1))
        o = torch.einsum("hij,jhd->ihd", s.softmax(-1), v.view(n, 8, 16)).reshape(n, 128)
        h = lay.norm1(h + o @ a.out_proj.weight.T + a.out_proj.bias)
        h = lay.norm2(h + lay.linear2(torch.relu(lay.linear1(h))))
    return m.fc(h)


@torch.no_grad()
def network(sd, tiles):
    """{B: (q_f64, q_f32)} of the class on the weights sd, or None when condition (a) or (b) fails."""
    m64, m32 = build(sd, torch.float64), build(sd, torch.float32)
    x64 = torch.from_numpy(tiles)
    rows = torch.cat([m64(x64[i:i + 1]) for i in range(max(SIZES))])
    out = {}
    for b in SIZES:
        q64, q32 = m64(x64[:b]), m32(x64[:b].float()).double()
        qmax, bound = float(q64.abs().max()), F32_FACTOR * float((q32 - q64).abs().max())
        assert float((spelled_out(m64, x64[:b]) - q64).abs().max()) <= 1e-9 * qmax
        quirk = float((q64 - rows[:b]).abs().max())
        moved = max(float((spelled_out(m64, x64[:b], NOISE, s) - q64).abs().max()) for s in range(3))
        print("  B %3d: max|Q| %.4g, f32 error %.3g, batch vs per-board rows %.3g, moved by logit noise %.3g (bound %.3g), all of max|Q|"
              % (b, qmax, bound / F32_FACTOR / qmax, quirk / qmax, moved / qmax, bound / qmax))
        if b == 1:
            assert quirk <= 1e-9 * qmax
        elif quirk <= 0.1 * qmax:
            return None
        if moved > bound / 4 or bound / F32_FACTOR >= 1e-5 * qmax:
            return None
        out[b] = (q64.numpy(), q32.numpy())
    return out


def main():
    torch.manual_seed(0)
    shapes = [(k, tuple(v.shape)) for k, v in HybridDQN().state_dict().items()]
    assert shapes == qw.reference_shapes()
    codes = np.load(os.path.join(HERE, "policy.npz"))["boards"]
    tiles = np.where(codes > 0, 2.0 ** codes.astype(np.float64), 0.0)
    print("online network, seed %d" % qw.SEED)
    online = network(qw.state_dict(shapes), tiles)
    assert online is not None, "the online network fails condition (a) or (b)"
    target, seed = None, 1
    while target is None:
        seed += 1
        print("target network, seed %d" % seed)
        target = network(qw.state_dict(shapes, seed=seed), tiles)
    i = np.arange(max(SIZES), dtype=np.int64)
    shaped = (((i * 37 + 11) % 101 - 20) / 4.0).astype(np.float32)
    dones = ((i * 7 + 3) % 5 == 0).astype(np.float32)
    out = {"sizes": np.array(SIZES, np.int64), "target_seed": np.int64(seed), "gamma": np.float64(GAMMA), "shaped": shaped, "dones": dones}
    for b in SIZES:
        (q64, q32), (t64, t32) = online[b], target[b]
        actions = q64.argmax(1)
        srt = np.sort(q64, axis=1)
        share = float(((srt[:, 3] - srt[:, 2]) <= 2 * F32_FACTOR * np.abs(q32 - q64).max()).mean())
        assert share <= TIE_CAP, (b, share)                                                   # (c)
        if b == 256:
            counts = np.bincount(actions, minlength=4)
            assert (counts >= 0.1 * b).sum() >= 2, counts                                     # (d)
            print("argmax counts at B 256: %s" % counts.tolist())
        out.update({"online_q_f64_%d" % b: q64, "online_q_f32_%d" % b: q32, "target_q_f64_%d" % b: t64, "target_q_f32_%d" % b: t32,
                    "actions_f64_%d" % b: actions.astype(np.int64),
                    "targets_f64_%d" % b: shaped[:b].astype(np.float64) + (1.0 - dones[:b]) * GAMMA * t64[np.arange(b), actions]})
    path = os.path.join(HERE, "qnet_batch.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes, target seed %d" % (path, os.path.getsize(path), seed))


if __name__ == "__main__":
    main()
