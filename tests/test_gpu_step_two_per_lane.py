"""The two-boards-per-lane step kernel (tune 2) at the sizes where a block of 512 boards is empty in its second pass, ragged in
its first, ragged in its second, or exactly full. Every lane of that kernel loads (a clamped index past the end) and computes;
only the stores are masked -- so what is checked is the oracle's results for the boards that exist, equality with the
one-board-per-lane kernel, and that nothing past board n is written in any output array."""
import numpy as np
import pytest

from test_gpu_step_matrix import ID_BASE, SEED, T0, assert_step, dev, same_tensors, start_scores

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (1, 256, 257, 511, 512, 513, 768, 769, 1025)
PAD = 600                       # more than a block of 512 boards past the end
STUCK = np.array([1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1], dtype=np.uint8)       # full, nothing merges: over whatever the move


@pytest.fixture(scope="module")
def ops():
    import torch
    import __graft_entry__ as ge
    ge.ensure_built()
    ge.import_package()
    from g2048 import ops as o
    assert torch.cuda.is_available()
    return o


@pytest.fixture(scope="module")
def cases(oracle):
    """Per size: boards (every fifth one and the last one stuck, so that games end and auto-reset runs at every size), scores, actions and the oracle's
    step with and without auto-reset. Computed once, read-only."""
    made = {}
    for n in SIZES:
        hb = oracle.synth_boards(n + PAD, seed=SEED, id_base=ID_BASE, p_empty=0.3, max_code=11)
        hb[::5] = STUCK
        hb[n - 1] = STUCK                                                          # the last board that exists, too
        hs = start_scores(n + PAD)
        ha = oracle.synth_actions(n + PAD, seed=SEED, step_index=T0, id_base=ID_BASE)
        want = {ar: oracle.step_batch(hb[:n], ha[:n], hs[:n], seed=SEED, step_index=T0, id_base=ID_BASE, opts=int(ar)) for ar in (False, True)}
        made[n] = (hb, hs, ha, want)
    assert all(int((made[n][3][True][3] & 1).sum()) >= (n + 4) // 5 for n in SIZES)          # games end: resets happen
    return made


@pytest.mark.parametrize("in_place", [False, True], ids=["separate", "inplace"])
@pytest.mark.parametrize("ar", [False, True], ids=["noar", "ar"])
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_two_per_lane_at_block_edges(ops, cases, f64, ar, in_place):
    import torch
    rdt = torch.float64 if f64 else torch.float32
    for n in SIZES:
        hb, hs, ha, want = cases[n]
        acts = dev(ha)
        got = {}
        for tune in (2, 1):
            src = dev(hb)
            if in_place:
                src[n:] = 0xAB
                out = src
            else:
                out = torch.full_like(src, 0xAB)
            sc = dev(hs.astype(np.int32))
            sc[n:] = 0x55AA55
            rw = torch.full((n + PAD,), -12345.0, dtype=rdt, device=DEV)
            fl = torch.full((n + PAD,), 0xEE, dtype=torch.uint8, device=DEV)
            o, r, f = ops.step(src[:n], acts[:n], sc[:n], SEED, T0, ID_BASE, out=out[:n], reward=rw[:n], flags=fl[:n],
                               reward_f64=f64, auto_reset=ar, tune=tune)
            torch.cuda.synchronize()
            what = (n, tune)
            assert_step(o, sc[:n], r, f, want[ar], f64, what)
            assert bool((out[n:] == 0xAB).all()) and bool((sc[n:] == 0x55AA55).all()), what
            assert bool((rw[n:] == -12345.0).all()) and bool((fl[n:] == 0xEE).all()), what
            if not in_place:
                assert bool((src == dev(hb)).all()), what             # the input is read only
            got[tune] = (out, sc, rw, fl)
        assert same_tensors(got[2], got[1]), n
