"""Guard bands (tests/guard.py) round every array the environment's entry points are handed (csrc/g2048_kernels.hip), and round
the hybrid agent's three small launches. Per entry point and size the same call is made twice from identical data, first with
bands of 0x00 and then with bands of 0xFF (NaN for floats, an index far out of range for integers) and the overwritten arrays
prefilled differently: (a) every band is intact after each call, (b) the two calls' outputs are equal bit for bit, (c) the
outputs are the reference's that the entry point's own test uses (the CPU oracle, or NumPy where that test restates it).

The last two tests are the proof that the harness sees an overrun end to end: a call on n + 1 rows into an output made for n.

The other families: tests/test_gpu_bounds_rollout.py, tests/test_gpu_bounds_per.py, tests/test_gpu_bounds_beam.py."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import guard
import qnet_beam_ref as QR
from conftest import tiles_of
from test_qnet_batch_host import torch_targets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x2048
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]        # the wavefront and the 256-thread block on both sides, and no multiple of anything
U8, I32, I64, F32, F64 = torch.uint8, torch.int32, torch.int64, torch.float32, torch.float64


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge
    ge.ensure_built()
    ge.import_package()
    from g2048 import ops as o, _lib
    _lib.lib()
    return o


def raw(name, *args):
    """The C entry point itself, where the wrapper allocates an output of its own."""
    from g2048 import _lib as L
    dev = torch.device(DEV)
    L.call(dev, getattr(L.lib(), name), *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], L.stream_ptr(dev))


def twice(call):
    return {k: v.numpy() for k, v in guard.twice(DEV, call).items()}


def boards_of(oracle, n, salt=0, p_empty=0.25, max_code=12):
    return oracle.synth_boards(n, seed=977 + salt, id_base=3 * n, p_empty=p_empty, max_code=max_code)


def same(a, b):
    return guard.same_bits(a, b)


# ------------------------------------------------------------------------------------------------------- one board a lane --
@pytest.mark.parametrize("n", SIZES)
def test_reset(ops, oracle, n):
    def call(s):
        b, sc = s.out("boards", n, (16,), U8, 16), s.out("scores", n, (), I32)
        ops.reset(n, SEED, 3, 77, boards=b, scores=sc)
        return {"boards": b, "scores": sc}
    got = twice(call)
    want_b, want_s = oracle.reset_batch(n, seed=SEED, epoch=3, id_base=77)
    assert np.array_equal(got["boards"], want_b) and np.array_equal(got["scores"].astype(np.uint32), want_s)


@pytest.mark.parametrize("agent", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_valid_moves(ops, oracle, n, agent):
    hb = boards_of(oracle, n, p_empty=0.1, max_code=4)
    got = twice(lambda s: {"mask": ops.valid_moves(s.inp("boards", hb, 16), agent, out=s.out("mask", n))})
    assert np.array_equal(got["mask"], oracle.valid_moves_batch(hb, agent))


@pytest.mark.parametrize("n", SIZES)
def test_evaluate_every_kind_with_and_without_phase(ops, oracle, n):
    hb = boards_of(oracle, n, 1, 0.2, 15)
    hb[0::3], hb[1::3] = np.minimum(hb[0::3], 8), np.minimum(hb[1::3], 9)             # boards of all three phases
    phase = (np.arange(n) % 3).astype(np.uint8)
    top = tiles_of(hb).max(axis=1)
    own_phase = np.where(top < 512, 0, np.where(top < 1024, 1, 2)).astype(np.uint8)     # _determine_game_phase (beam_search_agent.py)
    assert set(own_phase.tolist()) == {0, 1, 2} or n < 63
    for kind in range(11):
        for ph in (None, phase):
            def call(s):
                p = None if ph is None else s.inp("phase", ph)
                return {"out": ops.evaluate(s.inp("boards", hb, 16), kind, p, out=s.out("out", n, (), F64))}
            # (without a phase array EVAL_FULL takes the board's own phase; the other kinds never read one)
            assert same(twice(call)["out"], oracle.eval_batch(hb, kind, own_phase if ph is None else ph)), (kind, ph is not None)


@pytest.mark.parametrize("dtype,align", [(torch.float32, 16), (torch.float16, 8), (torch.bfloat16, 8)])
@pytest.mark.parametrize("n", SIZES)
def test_obs(ops, oracle, n, dtype, align):
    hb = boards_of(oracle, n, 2, 0.3, 17)
    got = guard.twice(DEV, lambda s: {"obs": ops.obs(s.inp("boards", hb, 16), out=s.out("obs", n, (16,), dtype, align))})["obs"]
    assert got.dtype == dtype and same(got, torch.from_numpy(oracle.obs_batch(hb)).to(dtype))


@pytest.mark.parametrize("n", SIZES)
def test_pack_and_unpack(ops, oracle, n):
    hb = boards_of(oracle, n, 3, 0.3, 17)
    tiles = oracle.unpack(hb).astype(np.int32).reshape(n, 16)
    got = twice(lambda s: {"tiles": ops.unpack(s.inp("boards", hb, 16), out=s.out("tiles", n, (16,), I32, 16))})
    assert np.array_equal(got["tiles"], tiles) and np.array_equal(tiles, tiles_of(hb))
    got = twice(lambda s: {"boards": ops.pack(s.inp("tiles", tiles, 16), out=s.out("boards", n, (16,), U8, 16))})
    assert np.array_equal(got["boards"], hb)


@pytest.mark.parametrize("n", SIZES)
def test_synth_boards_and_actions(ops, oracle, n):
    got = twice(lambda s: {"boards": ops.synth_boards(n, seed=3, id_base=2 ** 40, p_empty=0.05, max_code=17,
                                                      out=s.out("boards", n, (16,), U8, 16))})
    assert np.array_equal(got["boards"], oracle.synth_boards(n, seed=3, id_base=2 ** 40, p_empty=0.05, max_code=17))
    got = twice(lambda s: {"actions": ops.synth_actions(n, seed=SEED, step_index=9, id_base=12345, out=s.out("actions", n))})
    assert np.array_equal(got["actions"], oracle.synth_actions(n, seed=SEED, step_index=9, id_base=12345))


@pytest.mark.parametrize("n", SIZES)
def test_metrics_table(ops, oracle, n):
    """The output is a fixed table of 24 int64 that the kernel adds into: guarded as such, zeroed by the caller."""
    hb = boards_of(oracle, n, 4)
    sc = (np.arange(n) % 1000).astype(np.int32)
    fl = (np.arange(n) % 7 == 0).astype(np.uint8) | 0x02
    ex = (np.arange(n) % 31).astype(np.int32)

    def call(s):
        out = s.inp("out24", np.zeros(24, np.int64))
        ops.metrics(s.inp("boards", hb, 16), s.inp("scores", sc), s.inp("flags", fl), s.inp("expanded", ex), out=out)
        return {"out24": out}
    m = twice(call)["out24"]
    want = np.zeros(24, np.int64)
    want[:4] = n, sc.sum(), (fl & 1).sum(), ex.sum()
    want[4:22] = np.bincount(hb.max(axis=1), minlength=18)
    assert np.array_equal(m, want)


def track_reference(flags, expanded, alive, moves, valid, invalid, milestone, esum, move_index):
    """track_kernel restated (evaluate_beam_search.py:42-64): only games that are alive are touched."""
    live = alive != 0
    code = (flags >> 3).astype(np.int64)
    ms = milestone.copy()
    for k in range(8):
        ms[:, k] = np.where(live & (ms[:, k] < 0) & (code >= 6 + k), move_index, ms[:, k])
    ok = (flags & 2) != 0
    return (np.where(live & ((flags & 1) != 0), 0, alive).astype(np.uint8), moves + live, valid + (live & ok), invalid + (live & ~ok),
            ms, esum + np.where(live, expanded, 0))


@pytest.mark.parametrize("dyn", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_track_episodes(ops, n, dyn):
    rng = np.random.default_rng(n)
    flags = (rng.integers(0, 4, n) | (rng.integers(0, 15, n) << 3)).astype(np.uint8)
    expanded = rng.integers(0, 1000, n).astype(np.int32)
    alive = (rng.random(n) < 0.8).astype(np.uint8)
    moves, valid, invalid = (rng.integers(0, 50, n).astype(np.int32) for _ in range(3))
    milestone = np.where(rng.random((n, 8)) < 0.5, -1, rng.integers(0, 40, (n, 8))).astype(np.int32)
    esum = rng.integers(0, 1 << 40, n).astype(np.int64)
    words = np.zeros(16, np.int32)
    words[8] = 41                                       # the key block's move index

    def call(s):
        io = {"alive": s.inp("alive", alive), "moves": s.inp("moves", moves), "valid": s.inp("valid", valid),
              "invalid": s.inp("invalid", invalid), "milestone": s.inp("milestone", milestone, 16), "esum": s.inp("esum", esum)}
        kb = SimpleNamespace(words=s.inp("keyblock", words)) if dyn else None
        ops.track_episodes(s.inp("flags", flags), io["alive"], io["moves"], io["valid"], io["invalid"], io["milestone"], 41,
                           expanded=s.inp("expanded", expanded), expanded_sum=io["esum"], keyblock=kb)
        return io
    got = twice(call)
    want = track_reference(flags, expanded, alive, moves, valid, invalid, milestone, esum, 41)
    for k, w in zip(("alive", "moves", "valid", "invalid", "milestone", "esum"), want):
        assert np.array_equal(got[k], w), k


@pytest.mark.parametrize("dyn", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_sample_actions(ops, oracle, n, dyn):
    rng = np.random.default_rng(n + 1)
    probs = rng.dirichlet(np.ones(4), n).astype(np.float32)
    probs[: n // 8] = 0
    mask = rng.integers(0, 16, n).astype(np.uint8)
    words = np.zeros(16, np.uint32)
    words[6:8] = oracle.rng_keys(21, oracle.DOM_POLICY, 6)

    def call(s):
        kb = SimpleNamespace(words=s.inp("keyblock", words.view(np.int32))) if dyn else None
        a, p = ops.sample_actions(s.inp("probs", probs, 16), s.inp("mask", mask), seed=21, step_index=6, id_base=1000,
                                  actions=s.out("actions", n), prob=s.out("prob", n, (), F32), keyblock=kb)
        return {"actions": a, "prob": p}
    got = twice(call)
    oa, op = oracle.sample_batch(probs, mask, seed=21, step_index=6, id_base=1000)
    assert np.array_equal(got["actions"], oa) and same(got["prob"], op)


@pytest.mark.parametrize("n", SIZES)
def test_simulate_move(ops, oracle, n):
    hb = boards_of(oracle, n, 5, 0.35, 12)
    ha = oracle.synth_actions(n, seed=71)
    hc = np.maximum(hb.max(axis=1), (np.arange(n) % 5 + 9).astype(np.uint8))

    def call(s):
        o = {"succ": s.out("succ", n, (32, 16), U8, 16), "reward": s.out("reward", n, (32,), F64), "done": s.out("done", n, (32,), U8),
             "count": s.out("count", n)}
        raw("g2048_simulate_move", s.inp("boards", hb, 16), s.inp("actions", ha), s.inp("highest", hc), *o.values(), n)
        return o
    got = twice(call)
    for i in range(n):
        succ, r, d = oracle.simulate_move(tiles_of(hb[i]), int(ha[i]), 1 << int(hc[i]))
        k = succ.shape[0]
        assert got["count"][i] == k, i
        assert np.array_equal(tiles_of(got["succ"][i, :k]), succ) and same(got["reward"][i, :k], r), i
        assert np.array_equal(got["done"][i, :k], d.astype(np.uint8)), i
        assert not got["succ"][i, k:].any() and not got["reward"][i, k:].any() and not got["done"][i, k:].any(), i


@pytest.mark.parametrize("n", SIZES)
def test_simulate_move_sampled(ops, oracle, n):
    hb = np.concatenate([boards_of(oracle, n - n // 2, 6, 0.3, 12), boards_of(oracle, n // 2, 7, 0.85, 17)])
    ha = oracle.synth_actions(n, seed=31)

    def call(s):
        o = {"succ": s.out("succ", n, (8, 16), U8, 16), "reward": s.out("reward", n, (8,), F64), "done": s.out("done", n, (8,), U8),
             "count": s.out("count", n)}
        raw("g2048_simulate_move_sampled", s.inp("boards", hb, 16), s.inp("actions", ha), *o.values(), 77, 9, (1 << 40) + 3, n)
        return o
    got = twice(call)
    succ, rw, dn, cnt = oracle.hybrid_simulate_batch(hb, ha, seed=77, step_index=9, id_base=(1 << 40) + 3)
    assert np.array_equal(got["count"], cnt) and np.array_equal(got["succ"], succ)
    assert same(got["reward"], rw) and np.array_equal(got["done"], dn.astype(np.uint8))


# --------------------------------------------------------------------------------------------------- the other step forms --
@pytest.mark.parametrize("drawn", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_step_many(ops, oracle, n, drawn):
    """Three steps in one launch, the actions from a stream (f64 reward stream) or drawn in the kernel (f32 reward stream)."""
    steps, base, t0 = 3, 5 << 33, 7
    hb = boards_of(oracle, n, 8, 0.1, 6)
    hs = (np.arange(n) * 4).astype(np.int32)
    acts = np.stack([oracle.synth_actions(n, seed=SEED + 1 - drawn, step_index=t0 + t, id_base=base) for t in range(steps)])
    f64 = not drawn

    def call(s):
        sc = s.inp("scores", hs)
        o = {"out": s.out("out", n, (16,), U8, 16), "flags": s.out("flags", n), "rewards": s.out("rewards", steps, (n,), F64 if f64 else F32),
             "flags_stream": s.out("flags_stream", steps, (n,), U8), "episodes": s.out("episodes", n, (), I32), "scores": sc}
        ops.step_many(s.inp("boards", hb, 16), sc, SEED, t0, steps, base, out=o["out"], flags=o["flags"], reward_stream=o["rewards"],
                      flags_stream=o["flags_stream"], episodes=o["episodes"], reward_f64=f64, auto_reset=True,
                      actions=None if drawn else s.inp("actions", acts))
        return o
    got = twice(call)
    b, sc, episodes = hb, hs.astype(np.uint32), np.zeros(n, np.int32)
    for t in range(steps):
        b, sc, rw, fl = oracle.step_batch(b, acts[t], sc, seed=SEED, step_index=t0 + t, id_base=base, opts=1)
        assert same(got["rewards"][t], rw if f64 else rw.astype(np.float32)) and np.array_equal(got["flags_stream"][t], fl), t
        episodes += fl & 1
    assert np.array_equal(got["out"], b) and np.array_equal(got["scores"].astype(np.uint32), sc) and np.array_equal(got["flags"], fl)
    assert np.array_equal(got["episodes"], episodes)


@pytest.mark.parametrize("form", ["packed", "dyn"])
@pytest.mark.parametrize("n", SIZES)
def test_step_packed_and_dyn(ops, oracle, n, form):
    """The two other launch forms of the step kernel: the prepared call block (g2048_step_pack once, g2048_step_packed per call) and
    the keys from a device key block (g2048_step_dyn). PreparedStep runs step 0 once when it binds its arguments, so its scores
    carry two steps' gains."""
    base, t = 11, 5
    hb = boards_of(oracle, n, 12, 0.1, 5)
    ha = oracle.synth_actions(n, seed=SEED, step_index=t, id_base=base)
    hs = np.full(n, 8, np.int32)
    words = np.zeros(16, np.uint32)
    words[0:2], words[2:4] = oracle.rng_keys(SEED, oracle.DOM_STEP, t), oracle.rng_keys(SEED, oracle.DOM_EPISODE, t)

    def call(s):
        b, a, sc = s.inp("boards", hb, 16), s.inp("actions", ha), s.inp("scores", hs)
        o = {"out": s.out("out", n, (16,), U8, 16), "reward": s.out("reward", n, (), F64), "flags": s.out("flags", n), "scores": sc}
        if form == "packed":
            prepared = ops.PreparedStep(b, a, sc, SEED, base, out=o["out"], reward=o["reward"], flags=o["flags"], auto_reset=True)
            assert prepared.packed
            prepared(t)
        else:
            ops.step(b, a, sc, 0, 0, base, out=o["out"], reward=o["reward"], flags=o["flags"], reward_f64=True, auto_reset=True,
                     keyblock=SimpleNamespace(words=s.inp("keyblock", words.view(np.int32))))
        return o
    got = twice(call)
    sc = hs.astype(np.uint32)
    if form == "packed":
        _, sc, _, _ = oracle.step_batch(hb, ha, sc, seed=SEED, step_index=0, id_base=base, opts=1)
    b, sc, rw, fl = oracle.step_batch(hb, ha, sc, seed=SEED, step_index=t, id_base=base, opts=1)
    assert np.array_equal(got["out"], b) and np.array_equal(got["scores"].astype(np.uint32), sc)
    assert same(got["reward"], rw) and np.array_equal(got["flags"], fl)


def test_selftest_result_word(ops):
    got = twice(lambda s: (lambda r: (raw("g2048_selftest", r), {"result": r})[1])(s.out("result", 1, (), I32)))
    assert got["result"][0] == 0


@pytest.mark.parametrize("op", ["step", "reset"])
def test_env_step_record(ops, oracle, op):
    """One env, one launch, the 80-byte record (include/g2048.h: int32 tiles[16], score, flags, next mask, token, f64 reward)."""
    from g2048 import _lib as L
    hb = boards_of(oracle, 1, 9, 0.3, 9)
    action, token, index, board_id = 2, 0x1234, 17, 5

    def call(s):
        o = {"board": s.inp("board", hb, 16), "score": s.inp("score", np.array([40], np.int32)), "record": s.out("record", 1, (80,), U8, 16)}
        ops.env_step(o["board"], o["score"], o["record"].view(-1), SEED, index, board_id, action,
                     (L.ENV_OP_STEP if op == "step" else L.ENV_OP_RESET) | (token << L.ENV_TOKEN_SHIFT))
        return o
    got = twice(call)
    rec = got["record"].reshape(80)
    if op == "step":
        k0, k1 = oracle.rng_keys(SEED, oracle.DOM_STEP, index)
        tiles, score, reward, done, valid, _ = oracle.env_step(tiles_of(hb[0]), 40, action, oracle.rng_draw(k0, k1, board_id, 0))
    else:
        rb, _ = oracle.reset_batch(1, seed=SEED, epoch=index, id_base=board_id)
        tiles, score, reward, done, valid = tiles_of(rb[0]), 0, 0.0, False, False
    tiles = np.asarray(tiles, np.int32).reshape(16)
    assert np.array_equal(rec[:64].view(np.int32), tiles) and int(rec[64:68].view(np.int32)[0]) == score == int(got["score"][0])
    assert np.array_equal(tiles_of(got["board"][0]), tiles)
    assert (rec[68] & 1) == int(done) and ((rec[68] >> 1) & 1) == int(valid) and (1 << int(rec[68] >> 3)) == tiles.max()
    assert rec[69] == oracle.env_valid_mask(tiles) and int(rec[70:72].view(np.uint16)[0]) == token
    assert same(rec[72:80].view(np.float64), np.array([reward], np.float64))


@pytest.mark.parametrize("n", SIZES)
def test_replay_games(ops, oracle, n):
    """Ragged lengths 0 .. T; the histories are zeroed by the caller and written up to each game's end only."""
    T, base = 12, (3 << 33) + 17
    hb, _ = oracle.reset_batch(n, seed=99, epoch=0, id_base=base)
    acts = np.stack([oracle.synth_actions(n, seed=100, step_index=t, id_base=base) for t in range(T)], axis=1)      # (n, T)
    lens = (np.arange(n) % (T + 1)).astype(np.int32)
    hist = T + 1

    def call(s):
        o = {"boards_hist": s.inp("boards_hist", np.zeros((n, hist, 16), np.uint8), 16), "score_hist": s.inp("score_hist", np.zeros((n, hist), np.int32)),
             "flags_hist": s.inp("flags_hist", np.zeros((n, hist), np.uint8))}
        raw("g2048_replay_games", s.inp("boards0", hb, 16), None, None, base, s.inp("actions", acts), T, s.inp("n_moves", lens),
            *o.values(), hist, 99, n)
        return o
    got = twice(call)
    b, sc = hb, np.zeros(n, np.uint32)
    want = [np.zeros((n, hist, 16), np.uint8), np.zeros((n, hist), np.int32), np.zeros((n, hist), np.uint8)]
    for t in range(hist):
        at = lens >= t
        want[0][at, t], want[1][at, t] = b[at], sc[at].astype(np.int32)
        if t < T:
            b, sc, _, fl = oracle.step_batch(b, acts[:, t], sc, seed=99, step_index=t, id_base=base)
            want[2][lens > t, t] = fl[lens > t]
    for k, w in zip(got, want):
        assert np.array_equal(got[k], w), k


def test_keys_advance(ops, oracle):
    """The key block (16 words, ten of them written) and the counter behind it."""
    def call(s):
        o = {"words": s.inp("words", np.zeros(16, np.int32)), "counter": s.inp("counter", np.array([(1 << 32) + 41], np.int64))}
        raw("g2048_keys_advance", o["words"], o["counter"], SEED)
        return o
    got = twice(call)
    want = np.zeros(16, np.uint32)
    for at, dom in ((0, oracle.DOM_STEP), (2, oracle.DOM_EPISODE), (4, oracle.DOM_BEAM), (6, oracle.DOM_POLICY)):
        want[at:at + 2] = oracle.rng_keys(SEED, dom, (1 << 32) + 41)
    want[8:10] = 41, 1
    assert np.array_equal(got["words"].view(np.uint32), want) and int(got["counter"][0]) == (1 << 32) + 42


# ----------------------------------------------------------------------------------- the hybrid agent's small launches --
@pytest.mark.parametrize("n", SIZES)
def test_dqn_targets(ops, n):
    rng = np.random.default_rng(n + 2)
    qo, qt = (rng.normal(0, 3, (n, 4)).astype(np.float32) for _ in range(2))
    qo[::5, 1] = qo[::5, 3] = qo[::5].max(axis=1)                   # ties: the first maximum
    shaped, dones = rng.normal(0, 1, n).astype(np.float32), (rng.random(n) < 0.2).astype(np.float32)

    def call(s):
        t, a = ops.dqn_targets(s.inp("q_online", qo, 16), s.inp("q_target", qt, 16), s.inp("shaped", shaped), s.inp("dones", dones), 0.99,
                               targets=s.out("targets", n, (), F32), next_actions=s.out("next_actions", n, (), I64))
        return {"targets": t, "next_actions": a}
    got = twice(call)
    want_t, want_a = (t.numpy() for t in torch_targets(*(torch.from_numpy(x) for x in (qo, qt, shaped, dones)), 0.99))
    assert np.array_equal(got["next_actions"], want_a) and same(got["targets"], want_t)


@pytest.mark.parametrize("n", SIZES)
def test_qnet_select_actions(ops, oracle, n):
    """Epsilon 0: the exploit action, with `explored` all zero; epsilon 1: every board explores among its valid moves."""
    hb = boards_of(oracle, n, 10, 0.15, 8)
    q = np.random.default_rng(n + 3).normal(0, 1, (n, 4)).astype(np.float32)
    for eps in (0.0, 1.0):
        def call(s):
            a, e = ops.qnet_select_actions(s.inp("q", q, 16), s.inp("boards", hb, 16), eps, 5, 3, 1 << 40, actions=s.out("actions", n),
                                           explored=s.out("explored", n))
            return {"actions": a, "explored": e}
        got = twice(call)
        mask = oracle.valid_moves_batch(hb)
        if eps == 0.0:
            assert np.array_equal(got["actions"], [QR.exploit(q[i], hb[i]) for i in range(n)]) and not got["explored"].any()
        else:
            assert np.array_equal(got["explored"], (mask != 0).astype(np.uint8)) or got["explored"].all()
            assert (((mask >> got["actions"]) & 1) | (mask == 0)).all()


@pytest.mark.parametrize("n", SIZES)
def test_qnet_beam_expand(ops, oracle, n):
    hb = boards_of(oracle, n, 11, 0.3, 9)
    seed, step, base = 5, 3, (1 << 40) + 3

    def call(s):
        succ, count = ops.qnet_beam_expand(s.inp("boards", hb, 16), seed, step, base, succ=s.out("succ", n, (32, 16), U8, 16),
                                           count=s.out("count", n, (4,), U8, 4))
        return {"succ": succ, "count": count}
    got = twice(call)
    k0, k1 = oracle.rng_keys(seed, oracle.DOM_SIMULATE, step)
    for i in range(n):
        succ, count = QR.expand(hb[i], np.array([oracle.rng_draw(k0, k1, base + i, c) for c in range(12)], np.uint64).reshape(4, 3))
        assert np.array_equal(got["succ"][i], succ) and np.array_equal(got["count"][i], count), i


# ------------------------------------------------------------------------------------------- the harness sees an overrun --
def test_an_overrun_of_a_byte_output_is_seen(ops, oracle):
    """g2048_valid_moves on n + 1 boards with an output made for n: the kernel stores where it was told, inside the region's own
    allocation, and check() names the array, the band after the data and offset 0."""
    n = 256
    boards = guard.Region.of(np.full((n + 1, 16), 1, np.uint8), DEV, 16)        # every move but one is valid: no mask is 0x00 or 0xFF
    for byte in (0x00, 0xFF):
        out = guard.Region(n, (), U8, DEV).fill_bands(byte)
        raw("g2048_valid_moves", boards.view, out.view, n + 1, 0)
        torch.cuda.synchronize()
        band, offset, count = out.changed()
        assert (band, offset, count) == ("after", 0, 1)
        with pytest.raises(AssertionError, match=r"mask_out: the band after the data changed: first changed byte at offset 0 \("):
            out.check("mask_out")
        boards.check("boards")


def test_an_overrun_of_a_float_output_is_seen(ops, oracle):
    """The same for g2048_obs_f32: one row of sixteen floats past the end."""
    n = 63
    boards = guard.Region.of(np.full((n + 1, 16), 3, np.uint8), DEV, 16)
    for byte in (0x00, 0xFF):
        out = guard.Region(n, (16,), F32, DEV, 16).fill_bands(byte)
        raw("g2048_obs_f32", boards.view, out.view, n + 1)
        torch.cuda.synchronize()
        assert out.changed() == ("after", 0, 64)
        with pytest.raises(AssertionError, match=r"obs_out: the band after the data changed: first changed byte at offset 0 \("):
            out.check("obs_out")
        assert same(out.raw[out.hi:out.hi + 64].view(F32), np.full(16, np.float32(3) / np.float32(15), np.float32))
