"""CPU-side checks of the Q-network's batch forward (DeviceQNetwork.forward_batch, g2048_qnet_forward_batch) and of the
Double-DQN targets (g2048.dqn_targets): the plain-torch yardstick forward_batch_reference against the stock module's literal
batch call and against the reference class's recorded outputs (tests/golden/qnet_batch.npz), the conditions that make the
fixture a pin, the refusals, the C-ABI's argument validation without a device and the order of the targets' arithmetic. The
kernels themselves are checked on the GPU (tests/test_gpu_qnet_batch.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import qnet_weights as qw
from conftest import load_golden
from test_qnet_host import RefSpelling, golden_model, random_model, tiles

SIZES = (1, 17, 256, 300)
F32_FACTOR = 8.0


def target_model(g):
    """RefSpelling in float64 eval mode carrying the fixture's target-network weights."""
    model = RefSpelling(2048, 2).double()
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    model.load_state_dict({k: torch.from_numpy(v) for k, v in qw.state_dict(shapes, seed=int(g["target_seed"])).items()})
    return model.eval()


def torch_targets(q_online, q_target, shaped, dones, gamma):
    """hybrid.py:1042-1046 on given Q, the three lines of torch as the reference writes them."""
    next_actions = q_online.argmax(1, keepdim=True)
    next_q = q_target.gather(1, next_actions).squeeze(1)
    return shaped + (1 - dones) * gamma * next_q, next_actions.squeeze(1)


def test_forward_batch_reference_is_the_modules_literal_batch_call():
    from g2048 import qnet
    _, boards, model = golden_model()
    for name, m, b in (("fixture weights", model, boards), ("random init", random_model(2, 64, 2).double(), boards)):
        p = qnet.parse(m)
        for n in (1, 17, 256):
            with torch.no_grad():
                want = m(tiles(b[:n]))
            got = qnet.forward_batch_reference(p, torch.from_numpy(b[:n]))
            e = float((got - want).abs().max())
            print("%s n=%d: forward_batch_reference vs the module's batch call %.3g (max|Q| %.3g)" % (name, n, e, float(want.abs().max())))
            assert e <= 1e-9 * float(want.abs().max())
        one = qnet.forward_batch_reference(p, torch.from_numpy(b[:1]))
        assert float((one - qnet.forward_reference(p, torch.from_numpy(b[:1]))).abs().max()) <= 1e-12


def test_forward_batch_reference_reproduces_the_fixture():
    from g2048 import qnet
    g = load_golden("qnet_batch.npz")
    assert tuple(g["sizes"]) == SIZES and float(g["gamma"]) == 0.99
    _, boards, model = golden_model()
    for key, m in (("online", model), ("target", target_model(g))):
        p = qnet.parse(m)
        for n in SIZES:
            want = g["%s_q_f64_%d" % (key, n)]
            got = qnet.forward_batch_reference(p, torch.from_numpy(boards[:n])).numpy()
            assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), (key, n)
            f32 = qnet.forward_batch_reference(p, torch.from_numpy(boards[:n]), dtype=torch.float32).numpy()
            assert np.abs(f32 - want).max() <= 1e-4 * np.abs(want).max(), (key, n)


def test_fixture_pins_the_batch_function_actions_and_targets():
    g = load_golden("qnet_batch.npz")
    rows = load_golden("qnet.npz")["q_f64"]                     # the per-board function on the same boards and online weights
    shaped, dones = g["shaped"], g["dones"]
    assert shaped.dtype == np.float32 and dones.dtype == np.float32 and set(np.unique(dones)) == {0.0, 1.0}
    assert 0.1 < dones[:256].mean() < 0.9
    for n in SIZES:
        q, f32 = g["online_q_f64_%d" % n], g["online_q_f32_%d" % n]
        qmax = np.abs(q).max()
        quirk = np.abs(q - rows[:n]).max()
        if n == 1:
            assert quirk <= 1e-9 * qmax                          # one board: the same function
        else:
            assert quirk > 0.1 * qmax, "(a) the batch call no longer differs from the per-board rows"
        for key in ("online", "target"):                         # stock float32 is a fair yardstick on every case
            a, b = g["%s_q_f64_%d" % (key, n)], g["%s_q_f32_%d" % (key, n)]
            assert 0 < np.abs(a - b).max() < 1e-5 * np.abs(a).max()
        srt = np.sort(q, axis=1)
        assert ((srt[:, 3] - srt[:, 2]) <= 2 * F32_FACTOR * np.abs(f32 - q).max()).mean() <= 0.01, "(c) ties"
        actions = g["actions_f64_%d" % n]
        assert actions.dtype == np.int64 and np.array_equal(actions, q.argmax(1))
        want = shaped[:n].astype(np.float64) + (1.0 - dones[:n]) * 0.99 * g["target_q_f64_%d" % n][np.arange(n), actions]
        assert np.array_equal(g["targets_f64_%d" % n], want)
    counts = np.bincount(g["actions_f64_256"], minlength=4)
    assert (counts >= 0.1 * 256).sum() >= 2, "(d) %s" % counts


def test_forward_batch_refusals_name_their_reason():
    from g2048 import DeviceQNetwork, ops, qnet
    torch.manual_seed(4)
    b = torch.zeros((4, 16), dtype=torch.uint8)
    p4 = qnet.parse(RefSpelling(64, 1, nhead=4).eval())          # parse keeps accepting any head count ...
    assert p4.nhead == (4,) and p4.batch_first == (False,)
    with pytest.raises(ValueError, match="nhead 4, expected 8"):  # ... the batch function does not
        qnet.forward_batch_reference(p4, b)
    with pytest.raises(ValueError, match="nhead 4, expected 8"):
        qnet.check_batch_layers(p4)
    pbf = qnet.parse(RefSpelling(64, 2, batch_first=True).eval())
    assert pbf.batch_first == (True, True)
    with pytest.raises(ValueError, match="batch_first=True.*per-board"):
        qnet.check_batch_layers(pbf)
    ok = qnet.parse(RefSpelling(64, 2).eval())
    assert ok.nhead == (8, 8)
    qnet.check_batch_layers(ok)
    with pytest.raises(ValueError, match="training mode"):
        qnet.parse(RefSpelling(64, 2))

    class Stub(DeviceQNetwork):                                  # forward_batch's own checks, reached without a device
        def __init__(self, parsed, precision):
            self.parsed, self.precision = parsed, precision

    with pytest.raises(ValueError, match="bf16.*refused.*1e9"):
        Stub(ok, "bf16").forward_batch(b)
    with pytest.raises(ValueError, match="nhead 4"):
        Stub(p4, "f32").forward_batch(b)
    with pytest.raises(ValueError, match="batch_first=True"):
        Stub(pbf, "f32").forward_batch(b)
    import __graft_entry__ as ge
    ge.build()
    with pytest.raises(ValueError, match="1 .. 4096 boards.*not truncated"):
        ops.qnet_batch_workspace_bytes(4097, 64)
    with pytest.raises(ValueError, match="1 .. 4096"):
        ops.qnet_batch_workspace_bytes(0, 64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.qnet_forward_batch(b, torch.zeros(ops.qnet_plain_floats(64, 2)), 64, 2)


def test_batch_entry_points_validate_without_device():
    import __graft_entry__ as ge
    ge.build()
    from g2048 import _lib
    L = _lib.lib()
    assert _lib.QNET_BATCH_MAX == 4096
    hdr = open(__import__("os").path.join(__import__("conftest").REPO, "include", "g2048.h")).read()
    assert "#define G2048_QNET_BATCH_MAX 4096" in hdr
    # the workspace: x, qkv, att (128 + 384 + 128 floats a board) and the wider of the flattened conv output and the hidden layer,
    # boards rounded up to a tile of 16
    for ff in (32, 64, 2048, 4096, 96, 160, 224, 416):
        last = 0
        for n in (1, 15, 16, 17, 255, 256, 257, 1025, 4096):
            nb = L.g2048_qnet_batch_workspace(n, ff)
            assert nb == 4 * ((n + 15) // 16 * 16) * (640 + max(1024, ff)) and nb >= last and nb % 16 == 0
            last = nb
    for bad in ((0, 64), (4097, 64), (16, 48), (16, 0), (16, -32)):
        assert L.g2048_qnet_batch_workspace(*bad) == 0, bad
    buf = (C.c_uint8 * 256)()
    a = (C.addressof(buf) + 15) & ~15
    F = L.g2048_qnet_forward_batch
    assert F(None, None, None, 0, 64, 2, None, None) == 0                                     # n == 0: nothing to do
    for args in ((None, a, a, 8, 64, 2, a, None), (a, None, a, 8, 64, 2, a, None), (a, a, None, 8, 64, 2, a, None), (a, a, a, 8, 64, 2, None, None)):
        assert F(*args) == -1 and b"null pointer" in L.g2048_last_error()
    for args in ((a + 4, a, a, 8, 64, 2, a, None), (a, a + 8, a, 8, 64, 2, a, None), (a, a, a + 4, 8, 64, 2, a, None), (a, a, a, 8, 64, 2, a + 8, None)):
        assert F(*args) == -1 and b"misaligned" in L.g2048_last_error()
    assert F(a, a, a, 4097, 64, 2, a, None) == -1 and b"G2048_QNET_BATCH_MAX" in L.g2048_last_error()
    assert F(a, a, a, 8, 48, 2, a, None) == -1 and b"dim_ff" in L.g2048_last_error()
    assert F(a, a, a, 8, 64, 0, a, None) == -1 and b"n_layers" in L.g2048_last_error()
    T = L.g2048_dqn_targets
    assert T(None, None, None, None, 0.99, None, None, 0, None) == 0
    for i in range(6):
        ptrs = [a] * 6
        ptrs[i] = None
        assert T(ptrs[0], ptrs[1], ptrs[2], ptrs[3], 0.99, ptrs[4], ptrs[5], 8, None) == -1 and b"null pointer" in L.g2048_last_error()
    assert T(a + 4, a, a, a, 0.99, a, a, 8, None) == -1 and b"misaligned" in L.g2048_last_error()
    assert T(a, a, a, a, 0.99, a + 4, a, 8, None) == -1 and b"misaligned" in L.g2048_last_error()
    assert T(a, a, a, a, float("nan"), a, a, 8, None) == -1 and b"gamma" in L.g2048_last_error()


def test_targets_arithmetic_order_is_torchs():
    """float32, three roundings, no fused multiply-add: t = (1 - done) * gamma; t = t * next_q; target = shaped + t. The order
    g2048_dqn_targets follows, restated in NumPy and compared with the torch expression bit for bit."""
    g = load_golden("qnet_batch.npz")
    n = 300
    qo = g["online_q_f32_%d" % n].astype(np.float32)
    qt = g["target_q_f32_%d" % n].astype(np.float32)
    shaped, dones = g["shaped"][:n], g["dones"][:n]
    want, want_actions = torch_targets(torch.from_numpy(qo), torch.from_numpy(qt), torch.from_numpy(shaped), torch.from_numpy(dones), 0.99)
    actions = np.argmax(qo, axis=1)
    t = (np.float32(1.0) - dones) * np.float32(0.99)
    t = t * qt[np.arange(n), actions]
    got = shaped + t
    assert got.dtype == np.float32 and np.array_equal(got, want.numpy()) and np.array_equal(actions, want_actions.numpy())
    assert np.array_equal(got[dones == 1.0], shaped[dones == 1.0])
