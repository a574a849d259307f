"""Guard bands (tests/guard.py) round the arrays of the beam search's entry points (csrc/g2048_beam.hip): the decision of a batch
of roots at every block shape, the scratch of the depth-balanced order and the history of the previous call's order at exactly
the sizes the library states, and the complete games of one launch with all nine outputs and the helpers' workspace. The protocol
is tests/test_gpu_bounds.py's: two runs from identical data, bands of 0x00 and then of 0xFF, every band intact, the results
equal bit for bit and equal to the CPU oracle's, the reference of tests/test_gpu_beam.py and tests/test_gpu_evaluate.py."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import guard

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8, I32, I64, F32 = torch.uint8, torch.int32, torch.int64, torch.float32
DEPTH = 6


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge
    ge.ensure_built()
    return ge.import_package().ops


def raw(name, *args):
    from g2048 import _lib as L
    dev = torch.device(DEV)
    L.call(dev, getattr(L.lib(), name), *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], L.stream_ptr(dev))


def twice(call):
    return {k: v.numpy() for k, v in guard.twice(DEV, call).items()}


def roots_of(oracle, n, salt):
    """Ordinary boards, then a third of dead and nearly dead ones."""
    return np.concatenate([oracle.synth_boards(n - n // 3, seed=900 + salt, id_base=n, p_empty=0.2, max_code=17),
                           oracle.synth_boards(n // 3, seed=901 + salt, id_base=n, p_empty=0.0, max_code=3)])


def outputs(s, n):
    return {"action": s.out("action", n), "prob": s.out("prob", n, (), F32), "expanded": s.out("expanded", n, (), I32)}


def check_decisions(got, want, what=""):
    oa, op, oe = want
    assert np.array_equal(got["action" + what], oa) and guard.same_bits(got["prob" + what], op), what
    assert np.array_equal(got["expanded" + what].astype(np.uint32), oe), what


@pytest.mark.parametrize("width", [1, 20, 33, 128])            # one, two, four and eight wavefronts a game
@pytest.mark.parametrize("n", [1, 3, 65, 257])
def test_beam_get_action(ops, oracle, n, width):
    hb = roots_of(oracle, n, width)
    mask = oracle.valid_moves_batch(hb, False)
    seed, step, base = 21, 5, (1 << 33) + 9

    def call(s):
        o = outputs(s, n)
        ops.beam_get_action(s.inp("roots", hb, 16), width, DEPTH, s.inp("mask", mask), seed=seed, step_index=step, game_id_base=base,
                            out=tuple(o.values()))
        return o
    check_decisions(twice(call), oracle.beam_batch(hb, width, DEPTH, mask=mask, seed=seed, step_index=step, game_id_base=base))


@pytest.mark.parametrize("n", [3, 257])
def test_beam_get_action_dyn(ops, oracle, n):
    """g2048_beam_get_action_dyn: the search's keys from a device key block."""
    hb = roots_of(oracle, n, 5)
    words = np.zeros(16, np.uint32)
    words[4:6] = oracle.rng_keys(21, oracle.DOM_BEAM, 5)

    def call(s):
        o = outputs(s, n)
        ops.beam_get_action(s.inp("roots", hb, 16), 20, DEPTH, game_id_base=77, out=tuple(o.values()),
                            keyblock=SimpleNamespace(words=s.inp("keyblock", words.view(np.int32))))
        return o
    check_decisions(twice(call), oracle.beam_batch(hb, 20, DEPTH, seed=21, step_index=5, game_id_base=77))


def test_ranking_network_selftest(ops):
    """g2048_sort_selftest sorts in place: five waves of 64 keys and their 16 extra keys, as tests/test_gpu_beam.py checks it."""
    g = torch.Generator().manual_seed(5)
    n_waves = 5
    vals = (torch.randperm(1 << 24, generator=g)[: n_waves * 80] + 1).to(torch.int64)
    keys, extra = vals[: n_waves * 64].reshape(n_waves, 64), vals[n_waves * 64:].reshape(n_waves, 16)

    def call(s):
        k = s.inp("keys", keys.to(I32), 4)
        raw("g2048_sort_selftest", k, s.inp("extra", extra.to(I32), 4), n_waves, 32)
        return {"first48": k[:, :48].clone()}
    got = twice(call)
    assert np.array_equal(got["first48"], torch.sort(torch.cat([keys, extra], dim=1), dim=1, descending=True).values[:, :48].numpy())


@pytest.mark.parametrize("n", [4096, 5000])
def test_beam_get_action_with_the_order_scratch(ops, oracle, n):
    """g2048_beam_get_action_ws: the depth-balanced order is built in a scratch of exactly g2048_beam_workspace_bytes(n) bytes."""
    from g2048 import _lib as L
    hb = roots_of(oracle, n, 3)
    hb = hb[np.random.default_rng(n).permutation(n)]
    need = int(L.lib().g2048_beam_workspace_bytes(n))
    assert need == 4 * n

    def call(s):
        o = outputs(s, n)
        raw("g2048_beam_get_action_ws", s.inp("roots", hb, 16), None, *o.values(), 20, DEPTH, 512, 1024, 77, 3, 1000, n, 0,
            s.out("scratch", need, (), U8, 16), need)
        return o
    check_decisions(twice(call), oracle.beam_batch(hb, 20, DEPTH, seed=77, step_index=3, game_id_base=1000))


def test_beam_get_action_with_the_history(ops, oracle):
    """g2048_beam_get_action_hist: three consecutive call indices on a zeroed history of exactly g2048_beam_history_bytes(n) bytes;
    the second and the third call deal the games in the order the call before left there."""
    from g2048 import _lib as L
    n = 4096
    hb = roots_of(oracle, n, 4)
    hb = hb[np.random.default_rng(n).permutation(n)]
    need = int(L.lib().g2048_beam_history_bytes(n))
    assert need > 0

    def call(s):
        o = outputs(s, n)
        roots, hist = s.inp("roots", hb, 16), s.inp("history", np.zeros(need, np.uint8), 16)
        kept = {}
        for index in (1, 2, 3):
            for t in o.values():
                t.fill_(s.prefill)
            raw("g2048_beam_get_action_hist", roots, None, *o.values(), 20, DEPTH, 512, 1024, 5, 1, 0, n, 0, hist, need, index)
            kept.update({"%s%d" % (k, index): v.clone() for k, v in o.items()})
        return kept
    got = twice(call)
    want = oracle.beam_batch(hb, 20, DEPTH, seed=5, step_index=1, game_id_base=0)
    for index in (1, 2, 3):
        check_decisions(got, want, str(index))


def oracle_games(oracle, start, width, depth, cap, seed, base):
    """The games of one play launch, move by move: the oracle's beam decision (the agent's own valid moves) and env step for every
    game that is still alive."""
    n = len(start)
    b, sc = start.copy(), np.zeros(n, np.uint32)
    live = np.ones(n, bool)
    r = {"moves": np.zeros(n, np.int32), "valid": np.zeros(n, np.int32), "invalid": np.zeros(n, np.int32),
         "milestone": np.full((n, 8), -1, np.int32), "expanded": np.zeros(n, np.int64), "actions": np.full((n, cap), 0xFF, np.uint8)}
    for t in range(cap):
        a, _, ex = oracle.beam_batch(b, width, depth, seed=seed, step_index=t, game_id_base=base)
        nb, nsc, _, fl = oracle.step_batch(b, a, sc, seed=seed, step_index=t, id_base=base)
        b, sc = np.where(live[:, None], nb, b), np.where(live, nsc, sc)
        r["actions"][live, t] = a[live]
        r["expanded"] += np.where(live, ex, 0)
        r["moves"] += live
        r["valid"] += live & ((fl & 2) != 0)
        r["invalid"] += live & ((fl & 2) == 0)
        code = (fl >> 3).astype(np.int64)
        for k in range(8):
            r["milestone"][:, k] = np.where(live & (r["milestone"][:, k] < 0) & (code >= 6 + k), t, r["milestone"][:, k])
        live = live & ((fl & 1) == 0)
    r.update(boards=b, scores=sc, alive=live.astype(np.uint8))
    return r


@pytest.mark.parametrize("n,entry", [(40, "ws"), (300, "ws"), (40, "own"), (40, "tuned")])
def test_play_games_with_the_helpers_workspace(ops, oracle, n, entry):
    """g2048_play_games_ws: boards and scores in place, the seven result arrays (the n x max_moves action stream among them) and
    the helpers' workspace of exactly g2048_play_games_workspace(n) bytes, 64-byte aligned as the library asks. Also through
    g2048_play_games, which allocates that workspace itself, and g2048_play_games_tuned with the helpers' parameters given."""
    import ctypes
    from g2048 import _lib as L
    width, depth, cap, seed, base = 12, DEPTH, 24, 606, 500
    start, _ = oracle.reset_batch(n, seed=seed, epoch=0, id_base=base)
    start[: n // 4] = oracle.synth_boards(n // 4, seed=9, id_base=n, p_empty=0.02, max_code=3)       # crowded boards
    start[0] = (1 + (np.arange(16) + np.arange(16) // 4) % 2).astype(np.uint8)                       # a game that is over at once
    start[1] = start[0]
    start[1, 15] = 0                                                                                 # and one that is nearly
    need = int(L.lib().g2048_play_games_workspace(n))
    assert need >= n * 8 * 64
    tuning = (ctypes.c_uint32 * 4)(8, n, 2, 50)                     # eight helpers, every game registers at once

    def call(s):
        o = {"boards": s.inp("boards", start, 16), "scores": s.inp("scores", np.zeros(n, np.int32)), "moves": s.out("moves", n, (), I32),
             "valid": s.out("valid", n, (), I32), "invalid": s.out("invalid", n, (), I32), "milestone": s.out("milestone", n, (8,), I32, 16),
             "expanded": s.out("expanded", n, (), I64), "alive": s.out("alive", n), "actions": s.out("actions", n, (cap,), U8)}
        args = (*o.values(), width, depth, 512, 1024, cap, seed, base, n, 0)
        if entry == "own":
            raw("g2048_play_games", *args)
        else:
            ws = (s.out("workspace", need, (), U8, 64), need)
            raw("g2048_play_games_" + entry, *args, *ws, *((ctypes.cast(tuning, ctypes.c_void_p),) if entry == "tuned" else ()))
        return o
    got = twice(call)
    want = oracle_games(oracle, start, width, depth, cap, seed, base)
    assert 0 < want["alive"].sum() < n and want["moves"][0] == 1
    for k, w in want.items():
        assert np.array_equal(got[k].astype(w.dtype), w), k
