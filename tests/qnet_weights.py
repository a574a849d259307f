"""Weights of the hybrid Q-network fixture (tests/golden/qnet.npz), derived from a few integers with integer arithmetic only, so
that the 1,326,180 parameters need not be stored. The construction is that of tests/tpolicy_weights.py (whose functions this
module uses): element i of tensor number t is

    v = splitmix64((seed << 40) ^ (t << 32) ^ i) >> 48                  a 16-bit value
    w = (2 v - 65535) / 65536 * 2 ** exponent(t)    (+ 1 for a LayerNorm weight)

an odd multiple of 2**-16 in (-1, 1) times a per-tensor power of two: exact in float32. The exponents by kind of tensor
(RECIPE): every bias 1/32; LayerNorm weight 1 +- 0.25; a matrix or convolution with fan-in f the power of two next to
sqrt(3 / f) (f 4: 1, 128: 1/8, 1024: 1/16, 2048: 1/32), fc.weight 2 ** fc_gain_exp times that.
Shared by the generator and by the tests (the GPU machine rebuilds the exact network from it)."""
import numpy as np

import tpolicy_weights as tw
from tpolicy_weights import checksum  # noqa: F401

SEED = 1            # the first seed whose network meets the fixture conditions (gen_qnet_golden.py asserts them)
RECIPE = dict(seed=SEED, bias_exp=-5, norm_weight_exp=-2, fc_gain_exp=0)
N_PARAMETERS = 1326180


def exponent(name, shape):
    if ".norm" in name and name.endswith("weight"):
        return RECIPE["norm_weight_exp"]
    if name.endswith("bias"):
        return RECIPE["bias_exp"]
    e = tw.matrix_exp(int(np.prod(shape[1:])))
    return e + RECIPE["fc_gain_exp"] if name == "fc.weight" else e


def state_dict(named_shapes, seed=SEED):
    """{name: float64 array} for [(name, shape)] in state-dict order."""
    return tw.state_dict(named_shapes, seed, exponent)


def reference_shapes(dim_ff=2048, n_layers=2, prefix="transformer"):
    """(name, shape) of the reference's HybridDQN state dict, in its order."""
    out = [("cnn.0.weight", (32, 1, 2, 2)), ("cnn.0.bias", (32,)), ("cnn.2.weight", (64, 32, 2, 2)), ("cnn.2.bias", (64,)),
           ("embedding.weight", (128, 1024)), ("embedding.bias", (128,))]
    for l in range(n_layers):
        p = "%s.layers.%d." % (prefix, l)
        out += [(p + "self_attn.in_proj_weight", (384, 128)), (p + "self_attn.in_proj_bias", (384,)),
                (p + "self_attn.out_proj.weight", (128, 128)), (p + "self_attn.out_proj.bias", (128,)),
                (p + "linear1.weight", (dim_ff, 128)), (p + "linear1.bias", (dim_ff,)),
                (p + "linear2.weight", (128, dim_ff)), (p + "linear2.bias", (128,)),
                (p + "norm1.weight", (128,)), (p + "norm1.bias", (128,)), (p + "norm2.weight", (128,)), (p + "norm2.bias", (128,))]
    out += [("fc.weight", (4, 128)), ("fc.bias", (4,))]
    return out


def mask_bits(mask):
    """4-bit valid-move masks (bit a = action a valid) as a bool (N,4) array."""
    return ((np.asarray(mask).astype(np.int64)[:, None] >> np.arange(4)) & 1).astype(bool)


def masked_argmax(q, valid):
    """The exploit action of DQNAgent.select_action (agents/hybrid.py:947-953): Q of invalid moves replaced by -1e9, then
    np.argmax (ties to the lowest index). q (N,4) float, valid (N,4) bool."""
    return np.argmax(np.where(valid, q, np.asarray(-1e9, q.dtype)), axis=1).astype(np.uint8)


def top_two_gap(q, valid):
    """Per board the gap between the two largest Q-values among its valid moves (inf with fewer than two valid moves)."""
    m = np.sort(np.where(valid, np.asarray(q, np.float64), -np.inf), axis=1)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(m[:, 2]), m[:, 3] - m[:, 2], np.inf)
