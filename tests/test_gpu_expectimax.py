"""g2048_expectimax_actions on the device (include/g2048_search.h, ops.expectimax_actions) against the plain-Python restatement of
the definition (tests/expectimax_ref.py): == on every f64 value and every action at depths 1 to 3, over the boards the CPU test
holds the host build to; ragged sizes; a caller mask; no values; two calls; guard bands; the refusals."""
import numpy as np
import pytest
import torch

import expectimax_ref as R
import guard

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEG_INF = float("-inf")


@pytest.fixture(scope="module")
def g2048(oracle):
    import __graft_entry__ as ge
    ge.ensure_built()
    return ge.import_package()


def device_decide(boards, depth, mask=None, **kw):
    from g2048 import ops
    b = torch.as_tensor(np.array(boards), device=DEV)
    m = None if mask is None else torch.as_tensor(np.array(mask), device=DEV)
    a, v = ops.expectimax_actions(b, depth, m, want_values=True, **kw)
    torch.cuda.synchronize()
    return a.cpu().numpy(), v.cpu().numpy()


def same_f64(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_the_shared_boards_equal_the_restatement_bit_for_bit(g2048, depth):
    boards, want_a, want_v = R.reference(depth)
    got_a, got_v = device_decide(boards, depth)
    assert got_a.dtype == np.uint8 and got_v.dtype == np.float64
    assert np.array_equal(got_a, want_a), (got_a, want_a)
    assert same_f64(got_v, want_v), np.argwhere(got_v != want_v)
    names = list(R.HAND)
    row = lambda name: len(boards) - len(names) + names.index(name)      # noqa: E731
    assert got_a[row("dead")] == 0 and (got_v[row("dead")] == NEG_INF).all()
    assert int((got_v[row("one_move")] == NEG_INF).sum()) == 3
    if depth < 3:
        v = got_v[row("tie")]
        assert v[0] == v[2] == v.max() and got_a[row("tie")] == 0, "an exact tie goes to the lower action"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ragged_sizes(g2048, n):
    """Four boards a block: a lone board, ragged last blocks, and many blocks."""
    boards, want_a, want_v = R.reference(1, "ragged")
    got_a, got_v = device_decide(boards[:n], 1)
    assert np.array_equal(got_a, want_a[:n]) and same_f64(got_v, want_v[:n])


def test_a_caller_mask_removes_the_best_action(g2048):
    boards, want_a, want_v = R.reference(2)
    mask = (15 & ~(1 << want_a.astype(np.int64))).astype(np.uint8)
    ref_a, ref_v = R.decide(boards, 2, mask)
    got_a, got_v = device_decide(boards, 2, mask)
    assert np.array_equal(got_a, ref_a) and same_f64(got_v, ref_v)
    had_choice = np.isfinite(want_v).sum(axis=1) >= 2
    assert had_choice.sum() >= 8 and (got_a[had_choice] != want_a[had_choice]).all()
    assert (got_v[np.arange(len(boards)), want_a] == NEG_INF).all()
    # a mask of zero leaves no move: action 0 and four -inf
    got_a, got_v = device_decide(boards, 2, np.zeros(len(boards), np.uint8))
    assert (got_a == 0).all() and (got_v == NEG_INF).all()


def test_without_values_and_with_other_thresholds(g2048):
    from g2048 import ops
    boards, want_a, want_v = R.reference(1)
    b = torch.as_tensor(np.array(boards), device=DEV)
    only = ops.expectimax_actions(b, 1)
    assert isinstance(only, torch.Tensor) and only.dtype == torch.uint8 and np.array_equal(only.cpu().numpy(), want_a)
    assert np.array_equal(g2048.BatchedExpectimax(depth=1).get_actions(b).cpu().numpy(), want_a)
    ref_a, ref_v = R.decide(boards, 1, None, 64, 256)
    got_a, got_v = device_decide(boards, 1, early_threshold=64, mid_threshold=256)
    assert np.array_equal(got_a, ref_a) and same_f64(got_v, ref_v) and not same_f64(ref_v, want_v)


@pytest.mark.parametrize("depth,n", [(1, 65), (2, None)])
def test_guard_bands_and_two_calls_give_the_same_bits(g2048, depth, n):
    """Every array in guard bands, the outputs prefilled differently in two runs: nothing outside is written, nothing outside is
    read into a result, and the two runs agree bit for bit -- with the restatement too."""
    from g2048 import ops
    boards, want_a, want_v = R.reference(depth, "ragged" if n else "cases")
    boards, want_a, want_v = np.array(boards[:n]), want_a[:n], want_v[:n]
    mask = np.full(len(boards), 15, np.uint8)

    def call(s):
        b = s.inp("boards", boards, align=16)
        m = s.inp("mask", mask)
        a = s.out("actions", len(boards), (), torch.uint8)
        v = s.out("values", len(boards), (4,), torch.float64, align=8)
        ops.expectimax_actions(b, depth, m, actions=a, values=v)
        return {"actions": a, "values": v}

    out = guard.twice(DEV, call)
    assert np.array_equal(out["actions"].numpy(), want_a) and same_f64(out["values"].numpy(), want_v)

    def call_without_values(s):
        b = s.inp("boards", boards, align=16)
        a = s.out("actions", len(boards), (), torch.uint8)
        ops.expectimax_actions(b, depth, None, actions=a)
        return {"actions": a}

    assert np.array_equal(guard.twice(DEV, call_without_values)["actions"].numpy(), want_a)


def test_refusals_launch_nothing(g2048):
    """Bad arguments only: each gives the library's argument error, and the outputs keep their prefill."""
    from g2048 import _lib as L
    from g2048 import ops
    boards = torch.as_tensor(np.array(R.reference(1)[0]), device=DEV)
    n = boards.shape[0]
    actions = torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)
    values = torch.full((n, 4), 7.0, dtype=torch.float64, device=DEV)
    lib, fn = L.search_lib(), L.search_lib().g2048_expectimax_actions
    sp = L.stream_ptr(torch.device(DEV))
    for what, args, message in (
            ("depth 0", (boards.data_ptr(), None, actions.data_ptr(), values.data_ptr(), 0, 512, 1024, n, sp), "depth must be 1 .. 3"),
            ("depth 4", (boards.data_ptr(), None, actions.data_ptr(), values.data_ptr(), 4, 512, 1024, n, sp), "depth must be 1 .. 3"),
            ("misaligned boards", (boards.data_ptr() + 8, None, actions.data_ptr(), values.data_ptr(), 2, 512, 1024, n - 1, sp), "misaligned pointer"),
            ("a null output", (boards.data_ptr(), None, None, values.data_ptr(), 2, 512, 1024, n, sp), "null pointer")):
        assert fn(*args) == -1, what
        assert message in lib.g2048_search_last_error().decode(), what
        with pytest.raises(RuntimeError, match="g2048: g2048_expectimax_actions: "):
            L.search_call(torch.device(DEV), fn, *args)
    for depth in (0, 4):
        with pytest.raises(ValueError, match="depth must be 1 .. 3"):
            ops.expectimax_actions(boards, depth)
    torch.cuda.synchronize()
    assert bool((actions == 0xEE).all()) and bool((values == 7.0).all()), "a refused call reached the device"
    assert fn(None, None, None, None, 0, 0, 0, 0, sp) == 0, "n == 0 is a no-op"
