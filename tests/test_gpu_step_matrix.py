"""Every compiled step-kernel variant against the CPU oracle.

g2048_step / g2048_step_dyn / g2048_step_many pick a template instantiation from the opts bits and the batch size
(csrc/g2048_kernels.hip: step_impl, g2048_step_many). Each instantiation is compiled and scheduled on its own, so one can go
wrong while the others stay right. The instantiations are declared once below, as plain data, with how a call reaches each;
tests/test_abi_and_host.py checks (without a GPU) that they are exactly the ones the library holds.

Comparisons: boards, scores and flags equal; f64 rewards equal the oracle's bits; f32 rewards equal float32(oracle f64) bit
for bit; NaN equals NaN."""
import numpy as np
import pytest

# opts bits of include/g2048.h (plain ints, so that this module imports without a device)
F64, AR, RAND, NOOP = 0x01, 0x02, 0x04, 0x08

# step_kernel<REWARD_F64, AUTO_RESET, B, 256, RANDOM_ACTIONS, NOOP_ACTIONS>: (REWARD_F64, AUTO_RESET, B, RANDOM, NOOP), then the
# g2048_step opts bits and G2048_STEP_TUNE value that reach it. B = 2 is also what tune 0 picks from DEFAULT_B2_N boards on.
STEP_KERNELS = (
    ((False, False, 1, False, False), 0,                 1),
    ((True,  False, 1, False, False), F64,               1),
    ((False, True,  1, False, False), AR,                1),
    ((True,  True,  1, False, False), F64 | AR,          1),
    ((False, False, 2, False, False), 0,                 2),
    ((True,  False, 2, False, False), F64,               2),
    ((False, True,  2, False, False), AR,                2),
    ((True,  True,  2, False, False), F64 | AR,          2),
    ((False, False, 1, True,  False), RAND,              0),
    ((True,  False, 1, True,  False), RAND | F64,        0),
    ((False, True,  1, True,  False), RAND | AR,         0),
    ((True,  True,  1, True,  False), RAND | F64 | AR,   0),
    ((False, False, 1, False, True),  NOOP,              0),
    ((True,  False, 1, False, True),  NOOP | F64,        0),
    ((False, True,  1, False, True),  NOOP | AR,         0),
    ((True,  True,  1, False, True),  NOOP | F64 | AR,   0),
)
DEFAULT_B2_N = 2**22 + 1            # tune 0 picks two boards per lane from 2^22 boards on; + 1 leaves a ragged last block

# step_many_kernel<REWARD_F64, AUTO_RESET, 256, RANDOM>: (REWARD_F64, AUTO_RESET, RANDOM), then the g2048_step_many opts bits
STEP_MANY_KERNELS = (
    ((False, False, False), 0),
    ((True,  False, False), F64),
    ((False, True,  False), AR),
    ((True,  True,  False), F64 | AR),
    ((False, False, True),  RAND),
    ((True,  False, True),  RAND | F64),
    ((False, True,  True),  RAND | AR),
    ((True,  True,  True),  RAND | F64 | AR),
)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x5EED
T0 = 11                                     # step index of the first step of a chain
ID_BASE = (5 << 32) + 0x12345678            # high word set; no size below crosses the next multiple of 2^32
SIZES = (1, 255, 257, 511, 513, 70001)      # around the 256- and 512-board block tiles
DISTS = {"dense": (0.0, 3),                 # full boards of low codes: games end, auto-reset runs
         "sparse_huge": (0.7, 17),
         "mixed": (0.3, 11)}


def step_id(row):
    (f64, ar, b, rnd, noop), _, tune = row
    return "%s-%s-B%d-%s-tune%d" % ("f64" if f64 else "f32", "ar" if ar else "noar", b,
                                    "random" if rnd else "noop" if noop else "explicit", tune)


def many_id(row):
    (f64, ar, rnd), _ = row
    return "%s-%s-%s" % ("f64" if f64 else "f32", "ar" if ar else "noar", "random" if rnd else "explicit")


@pytest.fixture(scope="module")
def ops():
    import torch
    import __graft_entry__ as ge
    ge.ensure_built()
    ge.import_package()
    from g2048 import ops as o, _lib as L
    L.lib()
    assert torch.cuda.is_available()
    assert (F64, AR, RAND, NOOP) == (L.STEP_REWARD_F64, L.STEP_AUTO_RESET, L.STEP_RANDOM_ACTIONS, L.STEP_NOOP_ACTIONS)
    return o


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def host(t):
    return t.cpu().numpy()


def assert_rewards(got, want64, f64, what=""):
    g = host(got)
    w = want64 if f64 else want64.astype(np.float32)
    assert g.dtype == w.dtype, what
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan), what
    bits = np.uint64 if f64 else np.uint32
    assert np.array_equal(g.view(bits)[~nan], w.view(bits)[~nan]), what


def assert_step(out, sc, rw, fl, want, f64, what=""):
    bo, so, ro, fo = want
    assert np.array_equal(host(out), bo), what
    assert np.array_equal(host(sc).astype(np.uint32), so), what
    assert np.array_equal(host(fl), fo), what
    assert_rewards(rw, ro, f64, what)


def same_tensors(a, b):
    """Bit equality of two launches' outputs (rewards compared as integers: NaN payloads and -0.0 count)."""
    import torch
    for x, y in zip(a, b):
        if x.dtype in (torch.float32, torch.float64):
            it = torch.int32 if x.dtype == torch.float32 else torch.int64
            x, y = x.view(it), y.view(it)
        if not torch.equal(x, y):
            return False
    return True


def start_scores(n):
    return ((np.arange(n, dtype=np.uint64) * 36) % 4000).astype(np.uint32)


def host_actions(oracle, kind, n, t, id_base=ID_BASE):
    """The actions of step T0 + t: what the device gets (None = drawn in the kernel) and what the oracle gets."""
    if kind == "noop":                                       # bytes 0..8 and 255: above 3 moves nothing
        a = np.random.default_rng(1000 * n + t).integers(0, 10, n).astype(np.uint8)
        a[a == 9] = 255
        return a, a
    a = oracle.synth_actions(n, seed=SEED, step_index=T0 + t, id_base=id_base)
    return (None if kind == "random" else a), a


def unpack_row(row):
    (f64, ar, b, rnd, noop), opts, tune = row
    assert (bool(opts & F64), bool(opts & AR), bool(opts & RAND), bool(opts & NOOP)) == (f64, ar, rnd, noop)
    kind = "random" if rnd else "noop" if noop else "explicit"
    kw = dict(reward_f64=f64, auto_reset=ar, noop_actions=noop, tune=tune)
    oracle_opts = (1 if ar else 0) | (2 if noop else 0)
    return kind, kw, oracle_opts


def oracle_chain(oracle, hb, hs, kind, oracle_opts, steps, n, id_base=ID_BASE):
    want, acts = [], []
    for t in range(steps):
        da, ha = host_actions(oracle, kind, n, t, id_base)
        hb, hs, hr, hf = oracle.step_batch(hb, ha, hs, seed=SEED, step_index=T0 + t, id_base=id_base, opts=oracle_opts)
        want.append((hb, hs, hr, hf))
        acts.append(da)
    return want, acts


# ------------------------------------------------------------------------------------------------ g2048_step matrix --

@pytest.mark.parametrize("dist", sorted(DISTS))
@pytest.mark.parametrize("row", STEP_KERNELS, ids=step_id)
def test_step_kernel_vs_oracle(ops, oracle, row, dist):
    """Three chained steps of every size, out of place and in place; explicit and no-op rows again through g2048_step_dyn
    (equal to the scalar form); random and no-op rows again with tune 1 and 2 (a schedule only: equal to tune 0)."""
    import torch
    from g2048 import _lib as L
    kind, kw, oracle_opts = unpack_row(row)
    f64 = kw["reward_f64"]
    p_empty, max_code = DISTS[dist]
    for n in SIZES:
        hb0 = oracle.synth_boards(n, seed=SEED + max_code, id_base=ID_BASE, p_empty=p_empty, max_code=max_code)
        hs0 = start_scores(n)
        want, acts = oracle_chain(oracle, hb0, hs0, kind, oracle_opts, 3, n)
        if kw["auto_reset"] and dist == "dense" and n == SIZES[-1]:
            assert sum(int((w[3] & 1).sum()) for w in want) > 50     # the distribution ends games: resets happen
        for in_place in (False, True):
            cur = dev(hb0)
            sc = dev(hs0.astype(np.int32))
            for t in range(3):
                a = None if acts[t] is None else dev(acts[t])
                others = []
                if kind != "random":                                 # the key-block form of the same step
                    kb = ops.KeyBlock(SEED, start=T0 + t, device=DEV).advance()
                    b2, s2 = cur.clone(), sc.clone()
                    o2, r2, f2 = ops.step(b2, a, s2, 0, 0, ID_BASE, out=b2 if in_place else None, keyblock=kb, **kw)
                    others.append(("dyn", o2, s2, r2, f2))
                if kind != "explicit":                               # the tune bits select nothing here
                    for tune in (1, 2):
                        b2, s2 = cur.clone(), sc.clone()
                        o2, r2, f2 = ops.step(b2, a, s2, SEED, T0 + t, ID_BASE, out=b2 if in_place else None,
                                              **dict(kw, tune=tune))
                        others.append(("tune%d" % tune, o2, s2, r2, f2))
                out, rw, fl = ops.step(cur, a, sc, SEED, T0 + t, ID_BASE, out=cur if in_place else None, **kw)
                assert (out.data_ptr() == cur.data_ptr()) == in_place
                what = (n, in_place, t)
                assert_step(out, sc, rw, fl, want[t], f64, what)
                for name, o2, s2, r2, f2 in others:
                    assert same_tensors((o2, s2, r2, f2), (out, sc, rw, fl)), (name,) + what
                cur = out
    if kind == "random":                                             # no key-block form: refused, nothing written
        n = 1000
        b = dev(oracle.synth_boards(n, seed=SEED, id_base=ID_BASE))
        out = torch.full_like(b, 0xAB)
        sc = torch.full((n,), 0x55AA55, dtype=torch.int32, device=DEV)
        rw = torch.full((n,), -12345.0, dtype=torch.float64 if f64 else torch.float32, device=DEV)
        fl = torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)
        kb = ops.KeyBlock(SEED, start=T0, device=DEV).advance()
        rc = L.lib().g2048_step_dyn(b.data_ptr(), None, out.data_ptr(), sc.data_ptr(), rw.data_ptr(), fl.data_ptr(),
                                    kb.words.data_ptr(), L.u64(ID_BASE), n, row[1], L.stream_ptr(b.device))
        assert rc == -1 and b"RANDOM_ACTIONS" in L.lib().g2048_last_error()
        torch.cuda.synchronize()
        assert bool((out == 0xAB).all()) and bool((sc == 0x55AA55).all()) and bool((rw == -12345.0).all()) and bool((fl == 0xEE).all())


@pytest.mark.parametrize("row", [r for r in STEP_KERNELS if r[0][2] == 2], ids=step_id)
def test_step_default_dispatch_two_boards_per_lane(ops, oracle, row):
    """The B = 2 kernels as g2048_step picks them by itself (tune 0) at 2^22 + 1 boards: a ragged last block, every
    distribution in one batch, two steps (out of place, then in place), and the key-block form equal to the scalar one."""
    kind, kw, oracle_opts = unpack_row(row)
    kw["tune"] = 0
    n = DEFAULT_B2_N
    parts = np.array_split(np.arange(n), len(DISTS))
    hb0 = np.concatenate([oracle.synth_boards(len(p), seed=SEED + k, id_base=ID_BASE + int(p[0]), p_empty=DISTS[d][0],
                                              max_code=DISTS[d][1]) for k, (d, p) in enumerate(zip(sorted(DISTS), parts))])
    hs0 = start_scores(n)
    want, acts = oracle_chain(oracle, hb0, hs0, kind, oracle_opts, 2, n)
    cur, sc = dev(hb0), dev(hs0.astype(np.int32))
    for t in range(2):
        a = dev(acts[t])
        kb = ops.KeyBlock(SEED, start=T0 + t, device=DEV).advance()
        b2, s2 = cur.clone(), sc.clone()
        o2, r2, f2 = ops.step(b2, a, s2, 0, 0, ID_BASE, out=b2 if t else None, keyblock=kb, **kw)
        out, rw, fl = ops.step(cur, a, sc, SEED, T0 + t, ID_BASE, out=cur if t else None, **kw)
        assert_step(out, sc, rw, fl, want[t], kw["reward_f64"], t)
        assert same_tensors((o2, s2, r2, f2), (out, sc, rw, fl)), t
        cur = out


@pytest.mark.parametrize("n", [1, 65, 255, 257, 511, 513, 70001])
@pytest.mark.parametrize("row", STEP_KERNELS, ids=step_id)
def test_step_kernel_writes_nothing_past_the_last_board(ops, row, n):
    """Every instantiation, out of place and in place: each output array (the 8-byte f64 reward included) carries a sentinel
    tail past board n that has to survive the launch."""
    import torch
    kind, kw, _ = unpack_row(row)
    pad = 600
    boards = ops.synth_boards(n + pad, seed=3, id_base=ID_BASE, device=DEV)
    acts = dev(host_actions(None, "noop", n + pad, 0)[0]) if kind == "noop" else ops.synth_actions(n + pad, seed=3, device=DEV)
    rdt = torch.float64 if kw["reward_f64"] else torch.float32
    for in_place in (False, True):
        src = boards.clone()
        out = src if in_place else torch.full_like(src, 0xAB)
        if in_place:
            out[n:] = 0xAB
        sc = torch.full((n + pad,), 0x55AA55, dtype=torch.int32, device=DEV)
        rw = torch.full((n + pad,), -12345.0, dtype=rdt, device=DEV)
        fl = torch.full((n + pad,), 0xEE, dtype=torch.uint8, device=DEV)
        ops.step(src[:n], None if kind == "random" else acts[:n], sc[:n], 3, 1, ID_BASE, out=out[:n], reward=rw[:n],
                 flags=fl[:n], **kw)
        torch.cuda.synchronize()
        assert bool((out[n:] == 0xAB).all()) and bool((sc[n:] == 0x55AA55).all()), in_place
        assert bool((rw[n:] == -12345.0).all()) and bool((fl[n:] == 0xEE).all()), in_place
        assert not bool((fl[:n] == 0xEE).any()) and not bool((rw[:n] == -12345.0).any())      # and every board in range was written


# ---------------------------------------------------------------- a 2^32 cut whose halves pick different B --

CUT_BASE, CUT_N = 2**32 - 1000, 2**22 + 5000        # 1,000 boards at B = 1, then 2^22 + 4,000 at B = 2


def test_cut_at_2_to_32_with_mixed_boards_per_lane(ops, oracle):
    import torch
    from g2048 import _lib as L
    n = CUT_N
    parts = np.array_split(np.arange(n), len(DISTS))
    hb = np.concatenate([oracle.synth_boards(len(p), seed=SEED + k, id_base=CUT_BASE + int(p[0]), p_empty=DISTS[d][0],
                                             max_code=DISTS[d][1]) for k, (d, p) in enumerate(zip(sorted(DISTS), parts))])
    hs = start_scores(n)
    ha = oracle.synth_actions(n, seed=SEED, step_index=T0, id_base=CUT_BASE)
    b, a = dev(hb), dev(ha)
    want = {ar: oracle.step_batch(hb, ha, hs, seed=SEED, step_index=T0, id_base=CUT_BASE, opts=int(ar)) for ar in (False, True)}
    # explicit actions: f64 without auto-reset, f32 with it
    for f64, ar in ((True, False), (False, True)):
        sc = dev(hs.astype(np.int32))
        out, rw, fl = ops.step(b, a, sc, SEED, T0, CUT_BASE, reward_f64=f64, auto_reset=ar)
        assert_step(out, sc, rw, fl, want[ar], f64, (f64, ar))
    # in-kernel random actions (= synth_actions, which `ha` is) + auto-reset: the oracle, and the same ids as separate launches
    # cut elsewhere
    sc = dev(hs.astype(np.int32))
    out, rw, fl = ops.step(b, None, sc, SEED, T0, CUT_BASE, auto_reset=True)
    assert_step(out, sc, rw, fl, want[True], False, "random")
    sc2 = dev(hs.astype(np.int32))
    o2, r2, f2 = torch.empty_like(out), torch.empty_like(rw), torch.empty_like(fl)
    cuts = (0, 1000, 1000 + 3 * 2**20 + 7, n)
    for lo, hi in zip(cuts, cuts[1:]):
        ops.step(b[lo:hi], None, sc2[lo:hi], SEED, T0, CUT_BASE + lo, out=o2[lo:hi], reward=r2[lo:hi], flags=f2[lo:hi],
                 auto_reset=True)
    assert same_tensors((o2, sc2, r2, f2), (out, sc, rw, fl))
    # a call across the cut that is refused writes nothing, in either half
    def refused(opts, reward_offset=0):
        f64 = bool(opts & F64)
        out = torch.full_like(b, 0xAB)
        sc = torch.full((n,), 0x55AA55, dtype=torch.int32, device=DEV)
        rw = torch.full((n + 1,), -12345.0, dtype=torch.float64 if f64 else torch.float32, device=DEV)
        fl = torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)
        rc = L.lib().g2048_step(b.data_ptr(), a.data_ptr(), out.data_ptr(), sc.data_ptr(), rw.data_ptr() + reward_offset,
                                fl.data_ptr(), L.u64(SEED), L.u64(T0), L.u64(CUT_BASE), n, opts, L.stream_ptr(b.device))
        torch.cuda.synchronize()
        assert rc == -1, hex(opts)
        assert bool((out == 0xAB).all()) and bool((sc == 0x55AA55).all()), hex(opts)
        assert bool((rw == -12345.0).all()) and bool((fl == 0xEE).all()), hex(opts)
    refused(F64 | AR | 0x1000)                  # an unknown opts bit
    refused(F64 | (3 << 8))                     # tune 3
    refused(F64 | AR, reward_offset=4)          # an f64 reward array on a 4-byte boundary
    assert bool((b == dev(hb)).all())


# ------------------------------------------------------------------------------------------ g2048_step_many matrix --

def _many_actions(oracle, kind, n, steps, id_base):
    """(steps, n) explicit action bytes for the device (high bits set: only the low two count) and their low bits for the
    oracle; None + synth_actions for the in-kernel policy."""
    if kind == "random":
        return None, [oracle.synth_actions(n, seed=SEED, step_index=T0 + t, id_base=id_base) for t in range(steps)]
    a = np.random.default_rng(n + steps).integers(0, 256, (steps, n)).astype(np.uint8)
    return a, [a[t] & 3 for t in range(steps)]


def _many_vs_oracle(ops, oracle, row, hb0, hs0, id_base, steps=3):
    (f64, ar, rnd), opts = row
    assert (bool(opts & F64), bool(opts & AR), bool(opts & RAND)) == (f64, ar, rnd)
    n = hb0.shape[0]
    da, ha = _many_actions(oracle, "random" if rnd else "explicit", n, steps, id_base)
    acts = None if da is None else dev(da)
    sc = dev(hs0.astype(np.int32))
    out, flast, rs, fs, eps = ops.step_many(dev(hb0), sc, SEED, T0, steps, id_base, reward_f64=f64, auto_reset=ar,
                                            want_rewards=True, want_flags=True, want_episodes=True, actions=acts)
    hb, hs, done = hb0, hs0, np.zeros(n, np.int32)
    for t in range(steps):
        hb, hs, hr, hf = oracle.step_batch(hb, ha[t], hs, seed=SEED, step_index=T0 + t, id_base=id_base, opts=int(ar))
        assert np.array_equal(host(fs[t]), hf), (n, t)
        assert_rewards(rs[t], hr, f64, (n, t))
        done += hf & 1
    assert np.array_equal(host(out), hb) and np.array_equal(host(sc).astype(np.uint32), hs) and np.array_equal(host(flast), hf)
    assert np.array_equal(host(eps), done if ar else np.zeros_like(done))
    # in place, every optional output off: the same final boards, scores and last flags
    bi, sm = dev(hb0), dev(hs0.astype(np.int32))
    o2, fl2, r2, f2, e2 = ops.step_many(bi, sm, SEED, T0, steps, id_base, out=bi, reward_f64=f64, auto_reset=ar, actions=acts)
    assert o2 is bi and r2 is None and f2 is None and e2 is None
    assert same_tensors((bi, sm, fl2), (out, sc, flast))
    return acts, (out, sc, flast, rs, fs)


@pytest.mark.parametrize("dist", ["dense", "mixed"])
@pytest.mark.parametrize("row", STEP_MANY_KERNELS, ids=many_id)
def test_step_many_kernel_vs_oracle(ops, oracle, row, dist):
    """T = 3 steps with the reward and flags streams on, against the oracle; then with every optional output off, in place."""
    p_empty, max_code = DISTS[dist]
    for n in (1, 255, 257, 70001):
        hb0 = oracle.synth_boards(n, seed=SEED + 7, id_base=ID_BASE, p_empty=p_empty, max_code=max_code)
        _many_vs_oracle(ops, oracle, row, hb0, start_scores(n), ID_BASE)


@pytest.mark.parametrize("row", STEP_MANY_KERNELS, ids=many_id)
def test_step_many_ids_across_a_multiple_of_2_to_32(ops, oracle, row):
    """step_many hashes the full 64-bit id; g2048_step cuts its launch at the multiple of 2^32 and folds the high word in as a
    launch constant. Both must give the oracle's results for the same ids, step for step."""
    import torch
    (f64, ar, rnd), _ = row
    base, n, steps = 2**32 - 700, 5000, 3
    hb0 = oracle.synth_boards(n, seed=SEED + 8, id_base=base, p_empty=0.1, max_code=5)
    acts, (out, sc, flast, rs, fs) = _many_vs_oracle(ops, oracle, row, hb0, start_scores(n), base, steps)
    b, s = dev(hb0), dev(start_scores(n).astype(np.int32))
    rws, fls = [], []
    for t in range(steps):
        b, rw, fl = ops.step(b, None if acts is None else acts[t].contiguous(), s, SEED, T0 + t, base, reward_f64=f64,
                             auto_reset=ar)
        rws.append(rw); fls.append(fl)
    assert same_tensors((b, s, fls[-1], torch.stack(rws), torch.stack(fls)), (out, sc, flast, rs, fs))
