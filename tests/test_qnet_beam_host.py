"""CPU-side checks of the hybrid agent's beam search (g2048_qnet_beam_actions, g2048_qnet_beam_expand, g2048_play_qnet_beam_games,
DeviceQNetwork.act_beam and use_beam_search=True in g2048.evaluate_qnet): the plain restatement (tests/qnet_beam_ref.py) and the
kernels' own decision code compiled for the host (tests/hostsim_beam) equal every decision the reference recorded
(tests/golden/qnet_beam.npz), the C-ABI refuses every bad argument without touching a device and names the fault, and the Python
layer refuses what it cannot run. The kernels themselves are checked on the GPU (tests/test_gpu_qnet_beam.py)."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

import qnet_beam_ref as R
from conftest import REPO, load_golden

HB_DIR = os.path.join(REPO, "tests", "hostsim_beam")


@pytest.fixture(scope="module")
def golden():
    return load_golden("qnet_beam.npz")


@pytest.fixture(scope="module")
def hb():
    subprocess.check_call(["make", "-C", HB_DIR, "-s"])
    return C.CDLL(os.path.join(HB_DIR, "libg2048_hostsim_beam.so"))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from g2048 import _lib
    return _lib.lib()


def p(a, ty=C.c_uint8):
    return a.ctypes.data_as(C.POINTER(ty)) if a is not None else None


def leaf_as_q(leaf):
    """Leaf values (..., 32) in the layout of succ_q (..., 32, 4): the maximum first, the other three below it."""
    q = np.repeat(np.asarray(leaf, np.float32)[..., None], 4, axis=-1)
    q[..., 1:] -= np.float32(1.0)
    return np.ascontiguousarray(q)


# ------------------------------------------------------------------------------------------------- the restatement --
def test_restatement_equals_the_reference_at_depth_30(golden):
    boards, planned, action = golden["d30_board"], golden["d30_planned"], golden["d30_action"]
    threshold = int(golden["threshold"])
    assert np.array_equal(planned, np.array([R.planned(b, threshold) for b in boards], np.uint8))
    assert (action[:, planned == 0] == 255).all() and (action[:, planned == 1] < 4).all()
    for wi, w in enumerate(golden["d30_widths"]):
        got = np.array([R.action(b, int(w)) for b in boards[planned == 1]], np.uint8)
        assert np.array_equal(got, action[wi, planned == 1]), "width %d" % w
    assert set(np.unique(action[:, planned == 1])) == {0, 1, 2, 3}


def test_restatement_equals_the_reference_at_depth_1(golden):
    boards, gamma = golden["d1_board"], float(golden["gamma"])
    diff = 0
    for s in range(2):
        for i, b in enumerate(boards):
            succ, cnt = R.expand(b, golden["d1_h"][s, i])
            assert np.array_equal(succ, golden["d1_succ"][s, i]) and np.array_equal(cnt, golden["d1_count"][s, i]), (s, i)
            for wi, w in enumerate(golden["d1_widths"]):
                a = R.action(b, int(w), 1, gamma, golden["d1_leaf"][s, i])
                assert a == golden["d1_action"][s, wi, i], (s, w, i)
                assert R.action(b, int(w)) == golden["d1_action_d30"][wi, i]
                diff += a != golden["d1_action_d30"][wi, i]
    assert diff >= 0.25 * 4 * len(boards)                # depth 1 is a different decision, not a relabelling
    assert (golden["d1_action"][0] != golden["d1_action"][1]).any(axis=0).sum() >= 2      # and it depends on the draws


# --------------------------------------------------------------------------------- the kernels' code, on the host --
def test_device_decision_on_the_host_equals_the_reference_at_depth_30(hb, golden):
    boards, planned, action = np.ascontiguousarray(golden["d30_board"]), golden["d30_planned"], golden["d30_action"]
    n = len(boards)
    got = np.empty(n, np.uint8)
    hb.hb_planned(p(boards), C.c_uint32(int(golden["threshold"])), p(got), C.c_size_t(n))
    assert np.array_equal(got, planned)
    for thr, want in ((1, (boards > 0).sum(1) >= 8), (1 << 17, ((boards > 0).sum(1) >= 8) & (boards.max(1) >= 17)), (1 << 18, np.zeros(n, bool))):
        hb.hb_planned(p(boards), C.c_uint32(thr), p(got), C.c_size_t(n))
        assert np.array_equal(got.astype(bool), want), thr
    for wi, w in enumerate(list(golden["d30_widths"]) + [64]):
        hb.hb_actions(p(boards), C.c_uint32(int(w)), C.c_double(0.99), None, p(got), C.c_size_t(n))
        assert np.array_equal(got[planned == 1], action[min(wi, 6), planned == 1]), "width %d" % w


def test_device_decision_on_the_host_equals_the_reference_at_depth_1(hb, golden):
    boards = np.ascontiguousarray(golden["d1_board"])
    n = len(boards)
    got = np.empty(n, np.uint8)
    for s in range(2):
        q = leaf_as_q(golden["d1_leaf"][s])
        for wi, w in enumerate(golden["d1_widths"]):
            hb.hb_actions(p(boards), C.c_uint32(int(w)), C.c_double(float(golden["gamma"])), p(q, C.c_float), p(got), C.c_size_t(n))
            assert np.array_equal(got, golden["d1_action"][s, wi]), (s, w)


def test_device_expand_on_the_host_equals_the_reference(hb, golden, oracle):
    boards = np.ascontiguousarray(golden["d1_board"])
    n = len(boards)
    hb.hb_draw.restype = C.c_uint32
    hb.hb_draw.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32]
    for s in range(2):
        h = np.ascontiguousarray(golden["d1_h"][s])
        succ, count = np.empty((n, 32, 16), np.uint8), np.empty((n, 4), np.uint8)
        hb.hb_expand(p(boards), p(h, C.c_uint32), p(succ), p(count), C.c_size_t(n))
        assert np.array_equal(succ, golden["d1_succ"][s]) and np.array_equal(count, golden["d1_count"][s])
        # the draws are those of (seed, SIMULATE, step, id = row, 3 a + pick)
        seed, step = int(golden["seed"]), int(golden["d1_steps"][s])
        k0, k1 = oracle.rng_keys(seed, oracle.DOM_SIMULATE, step)
        for i in range(0, n, 17):
            for ctr in range(12):
                assert hb.hb_draw(seed, step, i, ctr) == h[i, ctr // 3, ctr % 3] == oracle.rng_draw(k0, k1, i, ctr)


# --------------------------------------------------------------------------------------------------------- the C-ABI --
def aligned_buffer():
    buf = (C.c_uint8 * 1024)()
    return buf, (C.addressof(buf) + 63) & ~63


def test_beam_actions_validates_without_device(lib):
    buf, a = aligned_buffer()

    def call(q=a, boards=a, succ_q=None, actions=a, planned=a, explored=a, width=15, depth=30, threshold=64, gamma=0.99, epsilon=0.25,
             n=100):
        return lib.g2048_qnet_beam_actions(q, boards, succ_q, actions, planned, explored, width, depth, threshold, gamma, epsilon, 7, 3,
                                           1 << 33, n, None)

    def refused(what, **kw):
        assert call(**kw) == -1 and what in lib.g2048_last_error(), (kw, lib.g2048_last_error())
        assert b"g2048_qnet_beam_actions" in lib.g2048_last_error()

    assert call(q=None, boards=None, actions=None, planned=None, explored=None, width=0, depth=0, n=0) == 0
    for k in ("q", "boards", "actions"):
        refused(b"null pointer", **{k: None})
    for k, off in (("q", 4), ("q", 8), ("boards", 8), ("boards", 1)):
        refused(b"misaligned", **{k: a + off})
    refused(b"misaligned", succ_q=a + 4, depth=1)
    for bad in (0, 65, -1):
        refused(b"beam_width", width=bad)
    for bad in (0, -1):
        refused(b"search_depth", depth=bad)
    for bad in (0, -64):
        refused(b"threshold", threshold=bad)
    for bad in (float("nan"), float("inf"), -float("inf")):
        refused(b"gamma", gamma=bad)
    refused(b"succ_q", depth=1)                                      # depth 1 needs the candidates' Q-values
    for bad in (-0.1, 1.5, float("nan")):
        refused(b"epsilon", epsilon=bad)
        refused(b"epsilon", epsilon=bad, planned=None, explored=None)


def test_beam_expand_validates_without_device(lib):
    buf, a = aligned_buffer()

    def call(boards=a, succ=a, count=a, n=100):
        return lib.g2048_qnet_beam_expand(boards, succ, count, 7, 3, 1 << 33, n, None)

    def refused(what, **kw):
        assert call(**kw) == -1 and what in lib.g2048_last_error(), (kw, lib.g2048_last_error())
        assert b"g2048_qnet_beam_expand" in lib.g2048_last_error()

    assert call(boards=None, succ=None, count=None, n=0) == 0
    for k in ("boards", "succ", "count"):
        refused(b"null pointer", **{k: None})
    for k, off in (("boards", 8), ("succ", 4), ("count", 2)):
        refused(b"misaligned", **{k: a + off})
    refused(b"too large", n=1 << 60)


def test_play_qnet_beam_games_validates_without_device(lib):
    from g2048 import _lib as L
    assert lib.g2048_play_qnet_beam_workspace(0) == lib.g2048_play_qnet_beam_workspace(1 << 20) >= 8
    buf, a = aligned_buffer()
    ws = lib.g2048_play_qnet_beam_workspace(100)

    def call(boards=a, score=a, packed=a, dim_ff=128, n_layers=2, moves=a, valid=a, invalid=a, ms=a, reward=a, alive=a, actions=a,
             max_moves=10, epsilon=0.25, width=15, depth=30, threshold=64, n=100, opts=L.POLICY_F32, max_waves=0, workspace=a,
             ws_bytes=ws):
        return lib.g2048_play_qnet_beam_games(boards, score, packed, dim_ff, n_layers, moves, valid, invalid, ms, reward, alive, actions,
                                              max_moves, epsilon, width, depth, threshold, 7, 0, n, opts, max_waves, workspace, ws_bytes,
                                              None)

    def refused(what, **kw):
        assert call(**kw) == -1 and what in lib.g2048_last_error(), (kw, lib.g2048_last_error())
        assert b"g2048_play_qnet_beam_games" in lib.g2048_last_error()

    assert call(boards=None, score=None, packed=None, workspace=None, width=0, depth=0, n=0) == 0      # nothing to play
    for k in ("boards", "score", "packed", "moves", "valid", "invalid", "ms", "alive", "workspace"):
        refused(b"null pointer", **{k: None})
    for k, off in (("boards", 8), ("packed", 4), ("ms", 8), ("score", 2), ("moves", 1), ("reward", 4), ("workspace", 4)):
        refused(b"misaligned", **{k: a + off})
    refused(b"unknown opts", opts=2)
    refused(b"unknown opts", opts=1 << 4)
    refused(b"max_moves", max_moves=0)
    for bad in (-0.1, 1.5, float("nan")):
        refused(b"epsilon", epsilon=bad)
    for bad in (0, 65, -3):
        refused(b"beam_width", width=bad)
    refused(b"search_depth", depth=0)
    refused(b"g2048_qnet_beam_actions", depth=1)                     # depth 1 is the stepwise form's, and the message names it
    refused(b"threshold", threshold=0)
    refused(b"dim_ff", dim_ff=48)
    refused(b"n_layers", n_layers=0)
    refused(b"workspace", ws_bytes=ws - 1)
    for precision in (L.POLICY_F32, L.POLICY_BF16):                  # everything in order up to the last check
        for width in (1, 64):
            refused(b"workspace", opts=precision, width=width, depth=2, threshold=1, reward=None, actions=None, ws_bytes=0)


def test_existing_entry_points_keep_their_signatures():
    from g2048 import _lib as L
    assert L.ABI_VERSION == 5
    assert len(L.SIGNATURES["g2048_play_qnet_games"][1]) == 22 and len(L.SIGNATURES["g2048_qnet_select_actions"][1]) == 10
    assert len(L.SIGNATURES["g2048_play_qnet_beam_games"][1]) == 25


# ------------------------------------------------------------------------------------------------------------ Python --
def fake_network():
    from g2048 import qnet as qnet_module
    net = object.__new__(qnet_module.DeviceQNetwork)
    net.precision, net.dim_ff, net.n_layers, net.packed, net.device = "f32", 32, 1, None, torch.device("cuda", 0)
    return net


def test_evaluate_qnet_refuses_depth_1_in_one_launch(lib):
    import g2048
    net = fake_network()
    with pytest.raises(ValueError, match="search_depth 1 .* fused=False"):
        g2048.evaluate_qnet(net, 4, use_beam_search=True, search_depth=1)
    with pytest.raises(ValueError, match="search_depth 1 .* fused=False"):
        g2048.evaluate_qnet(net, 4, use_beam_search=True, search_depth=1, fused=True)
    for bad in (dict(beam_width=0), dict(beam_width=65), dict(search_depth=0), dict(beam_search_threshold=0)):
        with pytest.raises(ValueError, match=list(bad)[0]):
            g2048.evaluate_qnet(net, 4, use_beam_search=True, **bad)
    sig = inspect.signature(g2048.evaluate_qnet).parameters
    assert [sig[k].default for k in ("use_beam_search", "beam_width", "search_depth", "beam_search_threshold")] == [False, 15, 30, 64]


def test_python_wrappers_refuse_what_they_cannot_run(lib):
    from g2048 import DeviceQNetwork, ops
    boards, scores = torch.zeros((4, 16), dtype=torch.uint8), torch.zeros(4, dtype=torch.int32)
    q = torch.zeros((4, 4))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.qnet_beam_actions(q, boards)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.qnet_beam_expand(boards)
    for bad in (dict(beam_width=0), dict(beam_width=65), dict(search_depth=0), dict(threshold=0), dict(gamma=float("nan")),
                dict(epsilon=1.5)):
        with pytest.raises(ValueError, match=list(bad)[0]):
            ops.qnet_beam_actions(q, boards, **bad)
    with pytest.raises(ValueError, match="succ_q"):
        ops.qnet_beam_actions(q, boards, search_depth=1)
    blob = torch.zeros(ops.qnet_packed_bytes("f32", 32, 1), dtype=torch.uint8)
    with pytest.raises(ValueError, match="search_depth"):
        ops.play_qnet_beam_games(boards, scores, blob, 32, 1, search_depth=1)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.play_qnet_beam_games(boards, scores, blob, 32, 1)
    # act keeps the signature tests/test_qnet_play_host.py pins; the search is act_beam, with the reference's settings as defaults
    assert list(inspect.signature(DeviceQNetwork.act).parameters) == ["self", "boards", "epsilon", "seed", "step_index", "id_base"]
    sig = inspect.signature(DeviceQNetwork.act_beam).parameters
    assert list(sig)[:6] == ["self", "boards", "epsilon", "seed", "step_index", "id_base"]
    assert [sig[k].default for k in ("epsilon", "beam_width", "search_depth", "beam_search_threshold", "gamma")] == [0.0, 15, 30, 64, 0.99]
