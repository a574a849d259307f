"""CPU-side checks of the transformer policy's evaluation (g2048_play_tpolicy_games, g2048.evaluate_policy with a
DeviceTransformerPolicy): the C-ABI refuses every bad argument without touching a device and names the fault, the workspace size
is a constant, and the Python layer refuses what it cannot run. The games themselves are checked on the GPU
(tests/test_gpu_tpolicy_play.py)."""
import ctypes as C

import pytest
import torch

from test_tpolicy_host import RefSpelling


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from g2048 import _lib
    return _lib.lib()


def test_play_tpolicy_games_validates_without_device(lib):
    from g2048 import _lib as L
    assert lib.g2048_play_tpolicy_workspace(0) == lib.g2048_play_tpolicy_workspace(1 << 20) >= 8
    buf = (C.c_uint8 * 1024)()
    a = (C.addressof(buf) + 63) & ~63
    ws = lib.g2048_play_tpolicy_workspace(100)
    masked = L.POLICY_F32 | (L.PLAY_POLICY_MASKED << L.PLAY_POLICY_MODE_SHIFT)

    def call(boards=a, score=a, packed=a, dim_ff=128, n_layers=2, moves=a, valid=a, invalid=a, ms=a, reward=a, alive=a, actions=a,
             max_moves=10, n=100, opts=masked, max_blocks=0, workspace=a, ws_bytes=ws):
        return lib.g2048_play_tpolicy_games(boards, score, packed, dim_ff, n_layers, moves, valid, invalid, ms, reward, alive, actions,
                                            max_moves, 7, 0, n, opts, max_blocks, workspace, ws_bytes, None)

    def refused(what, **kw):
        assert call(**kw) == -1 and what in lib.g2048_last_error(), (kw, lib.g2048_last_error())
        assert b"g2048_play_tpolicy_games" in lib.g2048_last_error()

    assert call(boards=None, score=None, packed=None, workspace=None, n=0) == 0            # nothing to play
    for k in ("boards", "score", "packed", "moves", "valid", "invalid", "ms", "alive", "workspace"):
        refused(b"null pointer", **{k: None})
    for k, off in (("boards", 8), ("packed", 4), ("ms", 8), ("score", 2), ("moves", 1), ("valid", 2), ("invalid", 2),
                   ("reward", 4), ("workspace", 4)):
        refused(b"misaligned", **{k: a + off})
    refused(b"unknown opts", opts=2)                                            # precision 2
    refused(b"unknown opts", opts=1 << 8)                                       # bits above the mode
    refused(b"unknown mode", opts=3 << L.PLAY_POLICY_MODE_SHIFT)
    refused(b"max_moves", max_moves=0)
    refused(b"max_moves", max_moves=-5)
    for bad in (dict(dim_ff=48), dict(dim_ff=0), dict(dim_ff=-32), dict(dim_ff=65536 + 32)):
        refused(b"dim_ff", **bad)
    for bad in (dict(n_layers=0), dict(n_layers=65), dict(n_layers=-1)):
        refused(b"n_layers", **bad)
    refused(b"workspace", ws_bytes=ws - 1)
    refused(b"workspace", ws_bytes=0)
    # the optional arrays may be absent: with everything else in order the call then gets as far as the device
    for mode in (L.PLAY_POLICY_MASKED, L.PLAY_POLICY_UNMASKED, L.PLAY_POLICY_GREEDY):
        for precision in (L.POLICY_F32, L.POLICY_BF16):
            refused(b"max_moves", opts=precision | (mode << L.PLAY_POLICY_MODE_SHIFT), reward=None, actions=None, max_moves=0)


def test_python_layer_refuses_what_it_cannot_run(lib):
    import g2048
    from g2048 import DeviceTransformerPolicy, ops
    model = RefSpelling(32, 1).eval()
    with pytest.raises(TypeError, match="DevicePolicy"):
        g2048.evaluate_policy(model)                       # a bare module, not a device policy
    with pytest.raises(TypeError, match="DevicePolicy"):
        g2048.evaluate_policy(None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        DeviceTransformerPolicy(model)                     # the module lives on the CPU
    boards, scores = torch.zeros((4, 16), dtype=torch.uint8), torch.zeros(4, dtype=torch.int32)
    for precision in ("f32", "bf16"):
        size = ops.tpolicy_packed_bytes(precision, 32, 1)
        with pytest.raises(RuntimeError, match="ROCm device"):
            ops.play_tpolicy_games(boards, scores, torch.zeros(size, dtype=torch.uint8), 32, 1, precision)
        for wrong in (size - 16, size + 16, ops.tpolicy_packed_bytes(precision, 64, 1)):
            with pytest.raises(ValueError, match="blob of %d bytes" % size):
                ops.play_tpolicy_games(boards, scores, torch.zeros(wrong, dtype=torch.uint8), 32, 1, precision)
    with pytest.raises(ValueError, match="dim_ff"):
        ops.play_tpolicy_games(boards, scores, torch.zeros(16, dtype=torch.uint8), 48, 1)
    with pytest.raises(ValueError, match="mode"):
        ops.play_tpolicy_games(boards, scores, torch.zeros(16, dtype=torch.uint8), 32, 1, mode="best")
    with pytest.raises(ValueError, match="precision"):
        ops.play_tpolicy_games(boards, scores, torch.zeros(16, dtype=torch.uint8), 32, 1, precision="f16")


def test_stepwise_driver_keeps_its_positional_call():
    """The yardstick loop takes the forward as a keyword after the arguments it always had."""
    import inspect
    from g2048.evaluate import _play_policy_stepwise
    names = list(inspect.signature(_play_policy_stepwise).parameters)
    assert names[:7] == ["env", "blob", "precision", "max_moves", "mode", "seed", "game_id_base"] and "forward" in names[7:]
