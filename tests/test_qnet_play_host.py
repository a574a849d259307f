"""CPU-side checks of the Q-network's evaluation (g2048_qnet_select_actions, g2048_play_qnet_games, g2048.evaluate_qnet): the
C-ABI refuses every bad argument without touching a device and names the fault, the workspace size is a constant, and the Python
layer refuses what it cannot run. The games themselves are checked on the GPU (tests/test_gpu_qnet_play.py)."""
import ctypes as C

import pytest
import torch

from test_qnet_host import RefSpelling


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from g2048 import _lib
    return _lib.lib()


def aligned_buffer():
    buf = (C.c_uint8 * 1024)()
    return buf, (C.addressof(buf) + 63) & ~63


def test_select_actions_validates_without_device(lib):
    buf, a = aligned_buffer()

    def call(q=a, boards=a, actions=a, explored=a, epsilon=0.25, n=100):
        return lib.g2048_qnet_select_actions(q, boards, actions, explored, epsilon, 7, 3, 1 << 33, n, None)

    def refused(what, **kw):
        assert call(**kw) == -1 and what in lib.g2048_last_error(), (kw, lib.g2048_last_error())
        assert b"g2048_qnet_select_actions" in lib.g2048_last_error()

    assert call(q=None, boards=None, actions=None, explored=None, n=0) == 0                 # nothing to select
    for k in ("q", "boards", "actions"):
        refused(b"null pointer", **{k: None})
    for k, off in (("q", 4), ("q", 8), ("boards", 8), ("boards", 1)):
        refused(b"misaligned", **{k: a + off})
    for bad in (-0.1, 1.5, float("nan"), float("inf"), -float("inf")):
        refused(b"epsilon", epsilon=bad)
        refused(b"epsilon", epsilon=bad, explored=None)


def test_play_qnet_games_validates_without_device(lib):
    from g2048 import _lib as L
    assert lib.g2048_play_qnet_workspace(0) == lib.g2048_play_qnet_workspace(1 << 20) >= 8
    buf, a = aligned_buffer()
    ws = lib.g2048_play_qnet_workspace(100)

    def call(boards=a, score=a, packed=a, dim_ff=128, n_layers=2, moves=a, valid=a, invalid=a, ms=a, reward=a, alive=a, actions=a,
             max_moves=10, epsilon=0.25, n=100, opts=L.POLICY_F32, max_waves=0, workspace=a, ws_bytes=ws):
        return lib.g2048_play_qnet_games(boards, score, packed, dim_ff, n_layers, moves, valid, invalid, ms, reward, alive, actions,
                                         max_moves, epsilon, 7, 0, n, opts, max_waves, workspace, ws_bytes, None)

    def refused(what, **kw):
        assert call(**kw) == -1 and what in lib.g2048_last_error(), (kw, lib.g2048_last_error())
        assert b"g2048_play_qnet_games" in lib.g2048_last_error()

    assert call(boards=None, score=None, packed=None, workspace=None, n=0) == 0            # nothing to play
    for k in ("boards", "score", "packed", "moves", "valid", "invalid", "ms", "alive", "workspace"):
        refused(b"null pointer", **{k: None})
    for k, off in (("boards", 8), ("packed", 4), ("ms", 8), ("score", 2), ("moves", 1), ("valid", 2), ("invalid", 2),
                   ("reward", 4), ("workspace", 4)):
        refused(b"misaligned", **{k: a + off})
    refused(b"unknown opts", opts=2)                                            # precision 2
    refused(b"unknown opts", opts=1 << 4)                                       # bits above the precision: opts carries no mode
    refused(b"unknown opts", opts=L.POLICY_BF16 | (L.PLAY_POLICY_GREEDY << L.PLAY_POLICY_MODE_SHIFT))
    refused(b"unknown opts", opts=1 << 8)
    refused(b"max_moves", max_moves=0)
    refused(b"max_moves", max_moves=-5)
    for bad in (-0.1, 1.5, float("nan")):
        refused(b"epsilon", epsilon=bad)
    for bad in (dict(dim_ff=48), dict(dim_ff=0), dict(dim_ff=-32), dict(dim_ff=65536 + 32)):
        refused(b"dim_ff", **bad)
    for bad in (dict(n_layers=0), dict(n_layers=65), dict(n_layers=-1)):
        refused(b"n_layers", **bad)
    refused(b"workspace", ws_bytes=ws - 1)
    refused(b"workspace", ws_bytes=0)
    # the optional arrays may be absent, and both ends of epsilon's range are legal: with everything else in order the call then
    # gets as far as the next check
    for precision in (L.POLICY_F32, L.POLICY_BF16):
        for epsilon in (0.0, 1.0):
            refused(b"workspace", opts=precision, epsilon=epsilon, reward=None, actions=None, ws_bytes=0)


def test_python_layer_refuses_what_it_cannot_run(lib):
    import g2048
    from g2048 import DeviceQNetwork, ops
    model = RefSpelling(32, 1).eval()
    with pytest.raises(TypeError, match="DeviceQNetwork"):
        g2048.evaluate_qnet(model)                         # a bare module, not a device network
    with pytest.raises(TypeError, match="DeviceQNetwork"):
        g2048.evaluate_qnet(None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        DeviceQNetwork(model)                              # the module lives on the CPU
    boards, scores = torch.zeros((4, 16), dtype=torch.uint8), torch.zeros(4, dtype=torch.int32)
    for precision in ("f32", "bf16"):
        size = ops.qnet_packed_bytes(precision, 32, 1)
        with pytest.raises(RuntimeError, match="ROCm device"):
            ops.play_qnet_games(boards, scores, torch.zeros(size, dtype=torch.uint8), 32, 1, precision)
        for wrong in (size - 16, size + 16, ops.qnet_packed_bytes(precision, 64, 1)):
            with pytest.raises(ValueError, match="blob of %d bytes" % size):
                ops.play_qnet_games(boards, scores, torch.zeros(wrong, dtype=torch.uint8), 32, 1, precision)
    size = ops.qnet_packed_bytes("f32", 32, 1)
    blob = torch.zeros(size, dtype=torch.uint8)
    with pytest.raises(ValueError, match="dim_ff"):
        ops.play_qnet_games(boards, scores, torch.zeros(16, dtype=torch.uint8), 48, 1)
    with pytest.raises(ValueError, match="precision"):
        ops.play_qnet_games(boards, scores, blob, 32, 1, precision="f16")
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="epsilon"):
            ops.play_qnet_games(boards, scores, blob, 32, 1, epsilon=bad)
        with pytest.raises(ValueError, match="epsilon"):
            ops.qnet_select_actions(torch.zeros((4, 4)), boards, bad)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.qnet_select_actions(torch.zeros((4, 4)), boards, 0.5)


class FakeQNetwork:
    """A DeviceQNetwork that never touched a device: enough for evaluate_qnet's argument checks, which come before any launch."""
    precision, dim_ff, n_layers, packed = "f32", 32, 1, None
    device = torch.device("cuda", 0)


def test_evaluate_qnet_checks_its_arguments_before_any_launch(lib):
    import g2048
    from g2048 import qnet as qnet_module
    net = object.__new__(qnet_module.DeviceQNetwork)
    for k in ("precision", "dim_ff", "n_layers", "packed", "device"):
        setattr(net, k, getattr(FakeQNetwork, k))
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="epsilon"):
            g2048.evaluate_qnet(net, 4, epsilon=bad)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="max_moves"):
            g2048.evaluate_qnet(net, 4, max_moves=bad)
    with pytest.raises(ValueError, match="histories need the fused driver"):
        g2048.evaluate_qnet(net, 4, fused=False, histories="best5")
    with pytest.raises(ValueError, match="lives on cuda:0, not cuda:1"):
        g2048.evaluate_qnet(net, 4, device="cuda:1")


def test_stepwise_driver_keeps_its_signature_and_takes_an_action_callable():
    import inspect
    from g2048.evaluate import _play_policy_stepwise
    names = list(inspect.signature(_play_policy_stepwise).parameters)
    assert names[:9] == ["env", "blob", "precision", "max_moves", "mode", "seed", "game_id_base", "check_every", "forward"]
    assert names[9:] == ["act"] and inspect.signature(_play_policy_stepwise).parameters["act"].default is None


def test_act_defaults_are_the_exploit_action():
    import inspect
    from g2048 import DeviceQNetwork
    sig = inspect.signature(DeviceQNetwork.act)
    assert list(sig.parameters) == ["self", "boards", "epsilon", "seed", "step_index", "id_base"]
    assert sig.parameters["epsilon"].default == 0.0 and sig.parameters["step_index"].default == 0
