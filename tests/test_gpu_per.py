"""The hybrid agent's prioritized replay on the device (csrc/g2048_per.hip, g2048.DeviceReplayBuffer) against what the reference's
own classes returned (tests/golden/per.npz) and against the NumPy restatement tests/per_ref.py, which tests/test_per_host.py holds
to that fixture on the CPU.

What is exact and what is not. The shaping, the priorities, the ring and the gathered batch are bit for bit the reference's. The
search is exact to the cdf the launch itself computed (stage test: np.cumsum / searchsorted of the launch's own probs_out; a
re-associated float64 sum of values totalling 1 moves an entry by at most size * 2^-52). The probabilities are float32 values of
p^alpha / sum: powf and the order of the sum differ from NumPy's in the last bits, so against the reference a draw within 2^-21 of
a reference cdf entry may land next door (a few float32 ulps of the probabilities accumulated to a cdf of at most 1), and probs /
weights are held to 8 x the reference's own float32 error against a float64 evaluation of its formula (the bound
tests/test_gpu_qnet.py uses for float32).

Measured on an MI355X over the fixture's eleven sample calls: probs 0.38 - 1.00 x and weights 0.40 - 3.73 x the reference's own
error (identical values where all priorities are equal); at most 1 of 256 draws within 2^-21 of a reference cdf entry and no index
different from the reference's; no draw left out by the stage test.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import per_ref as R
from conftest import REPO, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 256                      # G2048_PER_SCAN_TILE (asserted below)


@pytest.fixture(scope="module")
def g2048():
    import __graft_entry__ as ge
    ge.ensure_built()
    pkg = ge.import_package()
    assert pkg._lib.PER_SCAN_TILE == TILE
    return pkg


@pytest.fixture(scope="module")
def golden():
    return load_golden("per.npz")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- shaping --
@pytest.mark.parametrize("n", [1, 63, 64, 65, None])
def test_shaping_equals_the_reference(g2048, golden, n):
    n = len(golden["shape_out"]) if n is None else n
    got = g2048.ops.dqn_shape_rewards(dev(golden["shape_state"][:n]), dev(golden["shape_next"][:n]), dev(golden["shape_reward"][:n]))
    assert got.dtype == torch.float32 and np.array_equal(host(got), golden["shape_out"][:n])


# ------------------------------------------------------------------------------------------------- the scripted runs --
class Ring:
    """The ring through the entry points' wrappers alone (g2048.ops.per_*): the caller-owned arrays, size and head."""

    def __init__(self, g2048, capacity, alpha, seed=0x2048):
        self.ops, self.capacity, self.alpha, self.seed = g2048.ops, capacity, alpha, seed
        self.arrays = (torch.zeros((capacity, 16), dtype=torch.uint8, device=DEV), torch.zeros((capacity, 16), dtype=torch.uint8, device=DEV),
                       torch.zeros(capacity, dtype=torch.uint8, device=DEV), torch.zeros(capacity, dtype=torch.float32, device=DEV),
                       torch.zeros(capacity, dtype=torch.uint8, device=DEV), torch.zeros(capacity, dtype=torch.float32, device=DEV))
        self.size = self.head = self.samples = 0

    def push(self, boards, actions, rewards, next_boards, flags):
        self.size, self.head = self.ops.per_push(*self.arrays, self.size, self.head, boards, actions, rewards, next_boards, flags)

    def sample(self, batch, beta, u=None, sample_index=0):
        r = self.ops.per_sample(*self.arrays, self.size, self.head, self.alpha, beta, batch, seed=self.seed, sample_index=sample_index, u=u,
                                want_probs=True)
        return {k: host(v) for k, v in r.items()}

    def update_priorities(self, indices, td):
        self.ops.per_update_priorities(self.arrays[5], self.size, self.head, indices, td)

    def logical(self):
        """(states, next_states, actions, rewards, dones, priorities) in deque order, on the host."""
        order = (torch.arange(self.size, device=DEV) + self.head) % self.capacity
        return tuple(host(a[order]) for a in self.arrays)


class ClassRing(Ring):
    """The same through g2048.DeviceReplayBuffer."""

    def __init__(self, g2048, capacity, alpha, seed=0x2048):
        self.buf = g2048.DeviceReplayBuffer(capacity, alpha=alpha, device=DEV, seed=seed)
        self.capacity = capacity

    size = property(lambda self: len(self.buf))
    head = property(lambda self: self.buf.head)
    arrays = property(lambda self: self.buf._ring())

    def push(self, *a):
        self.buf.push(*a)

    def sample(self, batch, beta, u=None, sample_index=0):
        (st, ac, rw, nx, dn), idx, w, shaped, probs = self.buf.sample(batch, beta=beta, u=u, want_probs=True)
        return {k: host(v) for k, v in dict(states=st, actions=ac, rewards=rw, next_states=nx, dones=dn, indices=idx, weights=w,
                                            shaped=shaped, probs=probs).items()}

    def update_priorities(self, indices, td):
        self.buf.update_priorities(indices, td)


def replay(g2048, golden, r, make):
    """Run r of the fixture through a ring; per op the priorities after it, per sample also the ring before and after the call and
    what the call returned for the fixture's draws."""
    ring = make(g2048, int(golden["r%d_capacity" % r]), float(golden["r%d_alpha" % r]))
    pool = {k: golden["pool_" + k] for k in ("state", "next", "action", "reward", "done")}
    record = []
    for op in R.script(golden, r):
        rec = dict(op=op)
        if op["kind"] == R.PUSH:
            rows = op["rows"]
            # rewards as float64 on odd ops (rounded to float32 by the push, as torch.tensor(rewards, dtype=float32) does)
            rw = pool["reward"][rows].astype(np.float64) if op["k"] & 1 else pool["reward"][rows]
            # the flags byte as the step kernels write it: bit 0 = done, the other bits must be ignored
            flags = (pool["done"][rows] | 0x02 | (np.uint8(5) << 3)).astype(np.uint8)
            ring.push(dev(pool["state"][rows]), dev(pool["action"][rows]), dev(rw), dev(pool["next"][rows]), dev(flags))
        elif op["kind"] == R.SAMPLE:
            rec["before"] = ring.logical()
            rec["got"] = ring.sample(op["batch"], op["beta"], u=dev(op["u"]))
            rec["after"] = ring.logical()
        else:
            ring.update_priorities(dev(op["uidx"]), dev(op["td"]))
        rec["prio"] = ring.logical()[5]
        record.append(rec)
    return record


@pytest.fixture(scope="module")
def replayed(g2048, golden):
    return [replay(g2048, golden, r, Ring) for r in range(int(golden["runs"]))]


@pytest.fixture(scope="module")
def replayed_class(g2048, golden):
    return [replay(g2048, golden, r, ClassRing) for r in range(int(golden["runs"]))]


def check_priorities_and_contents(record):
    for rec in record:
        op = rec["op"]
        assert np.array_equal(rec["prio"], op["prio"]), "priorities after op %d" % op["k"]
        if op["kind"] == R.SAMPLE:
            st, nx, ac, rw, dn, _ = rec["before"]
            idx = op["idx"]
            assert np.array_equal(st[idx], op["sstate"]) and np.array_equal(nx[idx], op["snext"]), op["k"]
            assert np.array_equal(ac[idx], op["saction"]) and np.array_equal(rw[idx], op["sreward"]) and np.array_equal(dn[idx], op["sdone"])


def check_against_reference(record):
    """Fixture u in: the reference's indices, except for draws within 2^-21 of a reference cdf entry (at most 1 % of a call's)."""
    for rec in record:
        op = rec["op"]
        if op["kind"] != R.SAMPLE:
            continue
        near = R.near_cdf(R.cdf_of(op["probs"]), op["u"], 2.0 ** -21)
        differs = rec["got"]["indices"] != op["idx"]
        print("op %d: %d of %d draws near a reference cdf entry, %d indices differ" % (op["k"], near.sum(), len(near), differs.sum()))
        assert near.mean() <= 0.01
        assert not (differs & ~near).any(), (op["k"], np.flatnonzero(differs & ~near))


@pytest.mark.parametrize("r", range(4))
def test_push_and_update_equal_the_reference(replayed, r):
    check_priorities_and_contents(replayed[r])


@pytest.mark.parametrize("r", range(4))
def test_indices_against_the_reference(replayed, r):
    check_against_reference(replayed[r])


@pytest.mark.parametrize("r", range(4))
def test_probs_and_weights_within_8x_the_references_error(replayed, golden, r):
    alpha = float(golden["r%d_alpha" % r])
    for rec in replayed[r]:
        op = rec["op"]
        if op["kind"] != R.SAMPLE:
            continue
        got, prio = rec["got"], rec["before"][5]
        p64 = R.probs_f64(prio, alpha)
        perr = np.abs(got["probs"].astype(np.float64) - p64).max()
        w64 = R.weights_f64(p64, got["indices"], len(prio), op["beta"])
        werr = np.abs(got["weights"].astype(np.float64) - w64).max()
        print("run %d op %d: probs error %.3g = %.2f x the reference's %.3g; weights error %.3g = %.2f x the reference's %.3g" % (
            r, op["k"], perr, perr / op["perr"] if op["perr"] else np.inf if perr else 0.0, op["perr"],
            werr, werr / op["werr"] if op["werr"] else np.inf if werr else 0.0, op["werr"]))
        assert got["probs"].dtype == np.float32 and got["weights"].dtype == np.float32
        assert perr <= 8 * float(op["perr"]), (r, op["k"], perr, float(op["perr"]))
        assert werr <= 8 * float(op["werr"]), (r, op["k"], werr, float(op["werr"]))
        assert got["weights"].max() == np.float32(1.0)


@pytest.mark.parametrize("r", range(4))
def test_sample_gathers_shapes_and_leaves_the_buffer_alone(replayed, r):
    for rec in replayed[r]:
        if rec["op"]["kind"] != R.SAMPLE:
            continue
        got = rec["got"]
        for a, b in zip(rec["before"], rec["after"]):
            assert np.array_equal(a, b), "sample modified the buffer"
        st, nx, ac, rw, dn, prio = rec["before"]
        idx = got["indices"]
        assert idx.dtype == np.int64 and got["actions"].dtype == np.int64 and got["dones"].dtype == np.float32
        assert np.array_equal(got["states"], R.tiles_f32(st[idx])) and np.array_equal(got["next_states"], R.tiles_f32(nx[idx]))
        assert np.array_equal(got["actions"], ac[idx].astype(np.int64)) and np.array_equal(got["rewards"], rw[idx])
        assert np.array_equal(got["dones"], dn[idx].astype(np.float32))
        assert np.array_equal(got["shaped"], R.shaped_rewards(st[idx], nx[idx], rw[idx]))


@pytest.mark.parametrize("r", range(4))
def test_device_replay_buffer_runs_the_fixture_script(replayed_class, replayed, r):
    check_priorities_and_contents(replayed_class[r])
    check_against_reference(replayed_class[r])
    for a, b in zip(replayed_class[r], replayed[r]):                  # the class adds nothing to the entry points' results
        if a["op"]["kind"] == R.SAMPLE:
            assert a["got"].keys() == b["got"].keys()
            for k in a["got"]:
                assert np.array_equal(a["got"][k], b["got"][k]), k


# ------------------------------------------------------------------------------------------- scan and search, exact --
def filled_ring(g2048, size, head_kind, rng):
    """A ring of `size` live entries with random priorities written straight into the arrays. head_kind 0: head 0 in a ring with
    spare slots; 1: the logical order crosses the ring's end."""
    capacity = size + 5
    head = 0 if head_kind == 0 else capacity - min(2, size) if size > 1 else capacity - 1
    ring = Ring(g2048, capacity, 0.6)
    prio = np.exp(rng.normal(0.0, 1.5, size)).astype(np.float32)
    prio[rng.random(size) < 0.05] = np.float32(1e-5)
    slots = (head + np.arange(size)) % capacity
    full = [np.zeros((capacity, 16), np.uint8), np.zeros((capacity, 16), np.uint8), np.zeros(capacity, np.uint8),
            np.zeros(capacity, np.float32), np.zeros(capacity, np.uint8), np.full(capacity, 1e30, np.float32)]
    full[0][slots] = rng.integers(0, 12, (size, 16))
    full[1][slots] = rng.integers(0, 12, (size, 16))
    full[2][slots] = rng.integers(0, 4, size)
    full[3][slots] = rng.normal(0, 10, size).astype(np.float32)
    full[4][slots] = rng.integers(0, 2, size)
    full[5][slots] = prio
    ring.arrays = tuple(dev(a) for a in full)
    ring.size, ring.head = size, head
    return ring, prio


SCAN_SIZES = [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 64 * TILE + 1, 20000]


@pytest.mark.parametrize("head_kind", [0, 1])
@pytest.mark.parametrize("size", SCAN_SIZES)
def test_scan_and_search_are_exact_to_the_launchs_own_probs(g2048, size, head_kind):
    """indices == searchsorted(cumsum(float64(probs_out)) / last, u, 'right'), the only draws left out being those within
    size * 2^-52 of a cdf entry -- at most 0.1 % of them. 64 * TILE + 1 and 20,000 take more than one round of the wave that
    scans the tiles' sums; head_kind 1 reads the ring across its end."""
    rng = np.random.default_rng(1000 * size + head_kind)
    ring, prio = filled_ring(g2048, size, head_kind, rng)
    drawn = left_out = 0
    for batch in (1, 5, 256, 257):
        if batch > size:
            continue
        u = rng.random(batch)
        u[0] = 0.0 if batch > 1 else u[0]
        u[-1] = 1.0 - 2.0 ** -30
        got = ring.sample(batch, 0.4, u=dev(u))
        probs = got["probs"]
        assert probs.shape == (size,) and (probs > 0).all()
        p64 = R.probs_f64(prio, 0.6)
        assert np.abs(probs - p64).max() <= 1e-5 * p64.max()             # the right priorities in the right (logical) order
        cdf = R.cdf_of(probs)
        near = R.near_cdf(cdf, u, size * 2.0 ** -52)
        differs = got["indices"] != R.search(cdf, u)
        assert not (differs & ~near).any(), (batch, np.flatnonzero(differs & ~near))
        assert (got["indices"] >= 0).all() and (got["indices"] < size).all()
        drawn, left_out = drawn + batch, left_out + int(near.sum())
    assert left_out <= 0.001 * drawn, (left_out, drawn)


def test_size_below_batch_is_refused(g2048):
    ring, _ = filled_ring(g2048, 64, 0, np.random.default_rng(0))
    with pytest.raises(RuntimeError, match="fewer live entries"):
        ring.sample(65, 0.4)
    buf = g2048.DeviceReplayBuffer(10, device=DEV)
    with pytest.raises(ValueError, match="fewer than the batch"):
        buf.sample(1)
    z = torch.zeros((11, 16), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="capacity"):
        buf.push(z, z[:, 0].contiguous(), torch.zeros(11, device=DEV), z, z[:, 0].contiguous())
    assert len(buf) == 0


# --------------------------------------------------------------------------------------------------- counter draws --
@pytest.mark.parametrize("size,head_kind,batch", [(700, 0, 256), (2 * TILE + 1, 1, 257)])
def test_counter_draws_equal_explicit_draws(g2048, oracle, size, head_kind, batch):
    ring, _ = filled_ring(g2048, size, head_kind, np.random.default_rng(7))
    seed, index = 0x1234ABCD5678, 41
    ring.seed = seed
    k0, k1 = oracle.rng_keys(seed, R.DOM_REPLAY, index)
    h = np.array([oracle.rng_draw(k0, k1, j, 0) for j in range(batch)], dtype=np.uint64)
    u = h.astype(np.float64) * 2.0 ** -32
    assert len(np.unique(h)) > batch - 3 and u.max() < 1.0
    mine, explicit = ring.sample(batch, 0.7, sample_index=index), ring.sample(batch, 0.7, u=dev(u))
    other = ring.sample(batch, 0.7, sample_index=index + 1)
    for k in mine:
        assert np.array_equal(mine[k], explicit[k]), k
    assert not np.array_equal(mine["indices"], other["indices"])


# ------------------------------------------------------------------------------------------------------ properties --
def test_two_identical_calls_give_identical_bits(g2048):
    ring, _ = filled_ring(g2048, 20000, 1, np.random.default_rng(3))
    a, b = ring.sample(256, 0.4, sample_index=9), ring.sample(256, 0.4, sample_index=9)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def test_a_push_of_m_equals_m_pushes_of_one(g2048, golden):
    pool = {k: golden["pool_" + k] for k in ("state", "next", "action", "reward", "done")}
    one, many = Ring(g2048, 100, 0.6), Ring(g2048, 100, 0.6)
    args = lambda rows: (dev(pool["state"][rows]), dev(pool["action"][rows]), dev(pool["reward"][rows]), dev(pool["next"][rows]),    # noqa: E731
                         dev(pool["done"][rows]))
    for ring in (one, many):
        ring.push(*args(slice(0, 60)))
        idx = torch.arange(60, device=DEV)
        ring.update_priorities(idx, torch.linspace(0.0, 3.0, 60, device=DEV))          # distinct priorities
    many.push(*args(slice(60, 130)))                                                    # wraps: 30 evictions
    for i in range(60, 130):
        one.push(*args(slice(i, i + 1)))
    assert (one.size, one.head) == (many.size, many.head) == (100, 30)
    for a, b in zip(one.logical(), many.logical()):
        assert np.array_equal(a, b)
    assert (many.logical()[5][30:] == np.float32(3.0) + np.float32(1e-5)).all()
    many.push(*args(slice(130, 230)))                                                   # m == capacity: everything is replaced
    assert (many.size, many.head) == (100, 30) and np.array_equal(many.logical()[0], pool["state"][130:230])


def test_update_ignores_indices_beyond_the_live_entries_and_the_latest_duplicate_wins(g2048):
    ring, prio = filled_ring(g2048, 65, 1, np.random.default_rng(5))
    idx = np.array([3, 3, 64, 65, 69, -1, 3, 0, 64, 1 << 40], np.int64)
    td = np.arange(1, 11, dtype=np.float32)
    before = [host(a).copy() for a in ring.arrays]
    ring.update_priorities(dev(idx), dev(td))
    want = prio.copy()
    want[3], want[64], want[0] = np.float32(7) + np.float32(1e-5), np.float32(9) + np.float32(1e-5), np.float32(8) + np.float32(1e-5)
    assert np.array_equal(ring.logical()[5], want)
    dead = np.setdiff1d(np.arange(ring.capacity), (ring.head + np.arange(65)) % ring.capacity)
    assert np.array_equal(host(ring.arrays[5])[dead], before[5][dead])                  # no slot outside the live entries is written
    for a, b in zip(ring.arrays[:5], before[:5]):
        assert np.array_equal(host(a), b)


# ---------------------------------------------------------------------------------------------------- the example --
def test_example_runs(g2048):
    out = subprocess.run([sys.executable, os.path.join(REPO, "examples", "dqn_replay.py"), "--envs", "256", "--steps", "40"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "transitions/s" in out.stdout and "sample + update rounds" in out.stdout


def test_example_trains(g2048):
    """--train is the only place outside tests/test_gpu_qnet_train_round.py where the whole train_step runs in sequence; dim_ff 160
    runs a main group and a tail step of the products' contraction."""
    import re
    out = subprocess.run([sys.executable, os.path.join(REPO, "examples", "dqn_replay.py"), "--envs", "256", "--steps", "40", "--train",
                          "--dim-ff", "160"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rounds = re.search(r"with (\d+) sample \+ update rounds", out.stdout)
    loss = re.search(r"last weighted Huber loss (\S+)", out.stdout)
    assert rounds and int(rounds.group(1)) == 10 and loss, out.stdout[-2000:]
    assert np.isfinite(float(loss.group(1))) and float(loss.group(1)) >= 0, out.stdout[-2000:]
    prio = re.search(r"priorities (\S+) \.\. (\S+),", out.stdout)
    assert prio and all(np.isfinite(float(x)) and float(x) > 0 for x in prio.groups()), out.stdout[-2000:]
