"""Weights of the transformer-policy fixture (tests/golden/tpolicy.npz), derived from a few integers with integer arithmetic
only, so that the 702,213 parameters need not be stored: element i of tensor number t is

    v = splitmix64((seed << 40) ^ (t << 32) ^ i) >> 48                  a 16-bit value
    w = (2 v - 65535) / 65536 * 2 ** exponent(t)    (+ 1 for a LayerNorm weight)

i.e. an odd multiple of 2**-16 in (-1, 1) times a per-tensor power of two: exact in float32, no random stream of torch or NumPy
involved. The exponents by kind of tensor (RECIPE): embedding.weight 4.0; every bias 1/32; LayerNorm weight 1 +- 0.25; a matrix
with fan-in f the power of two next to sqrt(3 / f) (f 64: 1/4, 128: 1/8, 1024: 1/16, 2048: 1/32), the two heads 4 x that.
Shared by the generator and by the tests (the GPU machine rebuilds the exact network from it)."""
import zlib

import numpy as np

SEED = 1            # the first seed whose network meets the fixture conditions (gen_tpolicy_golden.py asserts them)
RECIPE = dict(seed=SEED, embedding_weight_exp=2, bias_exp=-5, norm_weight_exp=-2, head_gain_exp=2)
M64 = (1 << 64) - 1


def splitmix64(z):
    """splitmix64's output function on a uint64 array (wrapping arithmetic)."""
    z = z.astype(np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def matrix_exp(fan_in):
    """The exponent of the power of two next to sqrt(3 / fan_in): -((floor(log2 fan_in) - 1) // 2)."""
    return -((int(fan_in).bit_length() - 2) // 2)


def exponent(name, shape):
    if name == "embedding.weight":
        return RECIPE["embedding_weight_exp"]
    if ".norm" in name and name.endswith("weight"):
        return RECIPE["norm_weight_exp"]
    if name.endswith("bias"):
        return RECIPE["bias_exp"]
    e = matrix_exp(shape[-1])
    return e + RECIPE["head_gain_exp"] if name in ("actor.weight", "critic.weight") else e


def tensor(number, name, shape, seed=SEED, exponent=exponent):
    """Tensor `number` (its position in the state dict) as a float64 array; every value is exact in float32. exponent(name,
    shape): the per-tensor power of two (this module's, or another fixture's rule)."""
    count = int(np.prod(shape))
    key = np.uint64(((seed << 40) ^ (number << 32)) & M64)
    v = (splitmix64(key ^ np.arange(count, dtype=np.uint64)) >> np.uint64(48)).astype(np.int64)
    w = (2 * v - 65535).astype(np.float64) / 65536.0 * 2.0 ** exponent(name, shape)
    if ".norm" in name and name.endswith("weight"):
        w = w + 1.0
    return w.reshape(shape)


def state_dict(named_shapes, seed=SEED, exponent=exponent):
    """{name: float64 array} for [(name, shape)] in state-dict order."""
    return {name: tensor(i, name, tuple(shape), seed, exponent) for i, (name, shape) in enumerate(named_shapes)}


def checksum(arr):
    """CRC-32 of the tensor as little-endian float32 bytes."""
    return zlib.crc32(np.ascontiguousarray(arr, dtype="<f4").tobytes())


def reference_shapes(dim_ff=2048, n_layers=2, prefix="transformer_encoder"):
    """(name, shape) of the reference's TransformerModel state dict, in its order."""
    out = [("embedding.weight", (64, 1)), ("embedding.bias", (64,))]
    for l in range(n_layers):
        p = "%s.layers.%d." % (prefix, l)
        out += [(p + "self_attn.in_proj_weight", (192, 64)), (p + "self_attn.in_proj_bias", (192,)),
                (p + "self_attn.out_proj.weight", (64, 64)), (p + "self_attn.out_proj.bias", (64,)),
                (p + "linear1.weight", (dim_ff, 64)), (p + "linear1.bias", (dim_ff,)),
                (p + "linear2.weight", (64, dim_ff)), (p + "linear2.bias", (64,)),
                (p + "norm1.weight", (64,)), (p + "norm1.bias", (64,)), (p + "norm2.weight", (64,)), (p + "norm2.bias", (64,))]
    out += [("fc1.weight", (128, 1024)), ("fc1.bias", (128,)), ("fc2.weight", (64, 128)), ("fc2.bias", (64,)),
            ("actor.weight", (4, 64)), ("actor.bias", (4,)), ("critic.weight", (1, 64)), ("critic.bias", (1,))]
    return out
