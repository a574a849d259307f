"""Guard bands (tests/guard.py) for the entry points of the network side whose own tests carry no sentinel: the three weight
packers, whose output is a blob of exactly the size the library states, and the complete Q-network games with the beam search,
through the canary check the other three game-playing kernels already pass (tests/play_harness.py). The packers follow the
protocol of tests/test_gpu_bounds.py: two runs from identical data, bands of 0x00 and then of 0xFF, every band intact, the blobs
equal bit for bit and equal to the reference of tests/test_gpu_pack_blob.py (the documented layout assembled in NumPy); the PPO
network's blob, which has no such restatement, is held to the blob the forward tests use, packed into a tensor of its own."""
import numpy as np
import pytest
import torch

import guard
import play_harness as H
from play_harness import DEV, g2048  # noqa: F401
from test_gpu_pack_blob import SHAPES, qnet_case, tpolicy_case
from test_gpu_qnet_play import device_net

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("net", ["tpolicy", "qnet"])
def test_encoder_pack(g2048, net, precision, shape):
    from g2048 import ops
    dim_ff, layers = shape
    plain, want = (tpolicy_case if net == "tpolicy" else qnet_case)(precision == "bf16", dim_ff, layers)
    pack, size = (ops.tpolicy_pack, ops.tpolicy_packed_bytes) if net == "tpolicy" else (ops.qnet_pack, ops.qnet_packed_bytes)
    nb = size(precision, dim_ff, layers)
    got = guard.twice(DEV, lambda s: {"blob": pack(s.inp("plain", plain, 16), dim_ff, layers, precision, out=s.out("blob", nb, (), torch.uint8, 16))})
    assert np.array_equal(got["blob"].numpy().view(np.uint32), want)


@pytest.mark.parametrize("n_out", [4, 1])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_policy_pack(g2048, precision, n_out):
    from g2048 import ops
    plain = np.random.default_rng(n_out).normal(0, 0.3, 45504 + 65 * n_out).astype(np.float32)
    nb = ops.policy_packed_bytes(precision, n_out)
    got = guard.twice(DEV, lambda s: {"blob": ops.policy_pack(s.inp("plain", plain, 16), n_out, precision, out=s.out("blob", nb, (), torch.uint8, 16))})
    want = ops.policy_pack(torch.from_numpy(plain).to(DEV), n_out, precision)
    assert want.numel() == nb and torch.equal(got["blob"], want.cpu())
    assert len(np.unique(got["blob"].numpy())) > 16                          # (a blob of weights, not a fill)


def test_qnet_beam_games_canaries_and_one_move(g2048):
    """g2048_play_qnet_beam_games on n of n + 37 rows: nothing is written past n and the first n rows are the wrapper's."""
    H.check_canaries(H.QNET_BEAM, device_net("fixture", "f32"), (0.25, 15, 30, 64), [(77, 1), (300, 20)])
