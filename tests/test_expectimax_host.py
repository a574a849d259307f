"""The expectimax value function on the CPU: csrc/g2048_expectimax.h compiled for the host (tests/hostsim_expectimax, which
takes the four steps of the device's decide_wave in a plain loop) against the plain-Python restatement of the definition
(tests/expectimax_ref.py), == on every f64 and on every action; the hand-made edge boards; and the same host build with a
stand-alone driver under ASan + UBSan, run as a program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

import expectimax_ref as R

HX_DIR = os.path.join(REPO, "tests", "hostsim_expectimax")
NEG_INF = float("-inf")


@pytest.fixture(scope="module")
def hx(oracle):
    subprocess.check_call(["make", "-C", HX_DIR, "-s"])
    lib = C.CDLL(os.path.join(HX_DIR, "libg2048_hostsim_expectimax.so"))
    lib.hx_decide.restype = C.c_int
    lib.hx_decide.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.hx_value.restype = C.c_double
    lib.hx_value.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32]
    return lib


def host_decide(hx, boards, depth, mask=None, early=512, mid=1024):
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 16)
    n = len(boards)
    actions, values = np.full(n, 0xEE, np.uint8), np.full((n, 4), np.nan)
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    rc = hx.hx_decide(boards.ctypes.data, None if m is None else m.ctypes.data, depth, early, mid, n, actions.ctypes.data, values.ctypes.data)
    assert rc == 0
    return actions, values


def same_f64(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_host_build_equals_the_restatement_bit_for_bit(hx, depth):
    boards, want_a, want_v = R.reference(depth)
    assert len(boards) == {1: 64, 2: 16, 3: 4}[depth] + len(R.HAND)
    empty = (boards[:len(boards) - len(R.HAND)] == 0).sum(axis=1)
    assert depth == 1 or int(empty.max()) <= {2: 6, 3: 3}[depth]
    got_a, got_v = host_decide(hx, boards, depth)
    assert np.array_equal(got_a, want_a), (got_a, want_a)
    assert same_f64(got_v, want_v), np.argwhere(got_v != want_v)
    assert len(set(want_a.tolist())) >= 3, "the boards exercise fewer than three different decisions"


def test_hand_made_boards(hx, oracle):
    names = list(R.HAND)
    for depth in (1, 2, 3):
        boards, want_a, want_v = R.reference(depth)
        got_a, got_v = host_decide(hx, boards, depth)
        base = len(boards) - len(names)
        row = lambda name: base + names.index(name)      # noqa: E731
        # no move: action 0, as DeviceQNetwork.act answers, and four -inf
        assert oracle.valid_moves_batch(boards[row("dead")][None])[0] == 0
        assert got_a[row("dead")] == 0 and (got_v[row("dead")] == NEG_INF).all()
        # exactly one valid move: it is the decision, the other three are -inf
        only = int(oracle.valid_moves_batch(boards[row("one_move")][None])[0])
        assert bin(only).count("1") == 1 and got_a[row("one_move")] == only.bit_length() - 1
        assert int((got_v[row("one_move")] == NEG_INF).sum()) == 3
        # one merge on a full board: the moved board has ONE empty cell, so C is a sum of one pair divided by 1.0
        m = int(oracle.valid_moves_batch(boards[row("one_merge")][None])[0])
        assert (boards[row("one_merge")] != 0).all() and m == 0b0101
        for a in (0, 2):
            moved = oracle.env_move(oracle.unpack(boards[row("one_merge")][None])[0], a)[0]
            assert int((moved == 0).sum()) == 1
        # a 32768 tile takes part
        assert boards[row("code_15")].max() == 15 and np.isfinite(got_v[row("code_15")]).all()
    # the tie: LEFT and RIGHT are equal to the bit and the largest, and the lower index wins (depths 1 and 2)
    for depth in (1, 2):
        boards, want_a, want_v = R.reference(depth)
        i = len(boards) - len(names) + names.index("tie")
        got_a, got_v = host_decide(hx, boards[i][None], depth)
        v = got_v[0]
        assert v[0] == v[2] == v.max() and v[0] > v[1] and v[0] > v[3], v
        assert got_a[0] == 0 == want_a[i]


def test_a_caller_mask_removes_the_best_action(hx):
    boards, want_a, want_v = R.reference(1)
    boards = boards[:64]
    mask = (15 & ~(1 << want_a[:64].astype(np.int64))).astype(np.uint8)
    ref_a, ref_v = R.decide(boards, 1, mask)
    got_a, got_v = host_decide(hx, boards, 1, mask)
    assert np.array_equal(got_a, ref_a) and same_f64(got_v, ref_v)
    had_choice = np.isfinite(want_v[:64]).sum(axis=1) >= 2
    assert had_choice.sum() >= 32 and (got_a[had_choice] != want_a[:64][had_choice]).all()
    assert (got_v[np.arange(64), want_a[:64]] == NEG_INF).all()
    # what is left after the mask is what it was without it
    keep = np.isfinite(got_v)
    assert same_f64(got_v[keep], want_v[:64][keep])


def test_thresholds_reach_the_leaves(hx):
    """Another pair of thresholds changes the phase of boards between them, and both sides follow."""
    boards = R.boards_for(1)[:64]
    ref_a, ref_v = R.decide(boards, 1, None, 64, 256)
    got_a, got_v = host_decide(hx, boards, 1, None, 64, 256)
    assert np.array_equal(got_a, ref_a) and same_f64(got_v, ref_v)
    assert not same_f64(ref_v, R.reference(1)[2][:64])


def test_value_of_a_lane_is_the_restatements(hx, oracle):
    """ex_value<d>, what a lane computes for its successor, against Search.value for d = 0, 1, 2."""
    boards = R.boards_for(3)
    for d in (0, 1, 2):
        for b in boards:
            want = R.Search().value(tuple(int(x) for x in oracle.unpack(b[None])[0]), d)
            got = hx.hx_value(np.ascontiguousarray(b).ctypes.data, d, 512, 1024)
            assert got == want, (d, b, got, want)


def test_depth_outside_1_to_3_is_refused(hx):
    for depth in (0, 4, -1):
        assert hx.hx_decide(None, None, depth, 512, 1024, 0, None, None) == -1


def test_asan_ubsan_driver_runs_clean():
    """The host build and a stand-alone driver under -fsanitize=address,undefined, as tests/san does for the SWAR header: a
    program of its own, nothing loaded into Python."""
    subprocess.check_call(["make", "-C", HX_DIR, "-s", "expectimax_san"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([os.path.join(HX_DIR, "expectimax_san")], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "expectimax san ok: mismatches 0" in out.stdout
