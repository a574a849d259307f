"""ops.PreparedStep through the packed entry point (g2048_step_pack once, g2048_step_packed per call, on a side stream) against
ops.step with the same step index: bit for bit, at step indices below and above 2^32, for every plain variant; and the
fallback to g2048_step when the board ids cross a multiple of 2^32."""
import numpy as np
import pytest

from test_gpu_step_matrix import ID_BASE, SEED, same_tensors

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = (0, 7, 2**33 + 1)
STUCK = np.array([1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1], dtype=np.uint8)       # full, nothing merges


@pytest.fixture(scope="module")
def ops():
    import torch
    import __graft_entry__ as ge
    ge.ensure_built()
    ge.import_package()
    from g2048 import ops as o
    assert torch.cuda.is_available()
    return o


def run_both(ops, n, tune, f64, ar, id_base):
    """PreparedStep and ops.step on the same inputs for every step index; returns the PreparedStep."""
    import torch
    boards = ops.synth_boards(n, seed=SEED, id_base=id_base, device=DEV)
    boards[::5] = torch.tensor(STUCK, device=DEV)                 # games that end, so that auto-reset runs
    actions = ops.synth_actions(n, seed=SEED, id_base=id_base, device=DEV)
    start = (torch.arange(n, device=DEV, dtype=torch.int32) * 36) % 4000
    rdt = torch.float64 if f64 else torch.float32
    sc = start.clone()
    out, rw, fl = torch.empty_like(boards), torch.empty(n, dtype=rdt, device=DEV), torch.empty(n, dtype=torch.uint8, device=DEV)
    call = ops.PreparedStep(boards, actions, sc, SEED, id_base, out=out, reward=rw, flags=fl, auto_reset=ar, tune=tune)
    side = torch.cuda.Stream(device=DEV)
    for t in STEPS:
        sc.copy_(start)
        out.fill_(0xAB); rw.fill_(-12345.0); fl.fill_(0xEE)
        side.wait_stream(torch.cuda.current_stream(DEV))
        call(t, side.cuda_stream)
        side.synchronize()
        sc2 = start.clone()
        o2, r2, f2 = ops.step(boards, actions, sc2, SEED, t, id_base, reward_f64=f64, auto_reset=ar, tune=tune)
        torch.cuda.synchronize()
        assert same_tensors((out, sc, rw, fl), (o2, sc2, r2, f2)), (n, tune, f64, ar, t)
        assert not bool((fl == 0xEE).any()) and int((fl & 1).sum()) >= n // 5
    return call


@pytest.mark.parametrize("ar", [False, True], ids=["noar", "ar"])
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("tune", [0, 1, 2])
@pytest.mark.parametrize("n", [513, 70001])
def test_prepared_step_equals_step(ops, n, tune, f64, ar):
    assert run_both(ops, n, tune, f64, ar, ID_BASE).packed


@pytest.mark.parametrize("tune", [0, 2])
def test_prepared_step_falls_back_across_2_to_32(ops, tune):
    call = run_both(ops, 513, tune, False, True, 2**32 - 300)
    assert not call.packed
    assert run_both(ops, 513, tune, True, False, 2**32 - 513).packed          # ends exactly at the multiple: one launch
