"""Guard bands (tests/guard.py) round the arrays of the prioritized replay's entry points (csrc/g2048_per.hip): the six ring arrays,
the hand-carved workspaces at exactly the size the library states, and every output. The protocol is tests/test_gpu_bounds.py's:
two runs from identical data, bands of 0x00 and then of 0xFF, every band intact, the results equal bit for bit, and equal to the
reference of tests/test_gpu_per.py (tests/per_ref.py). Here the ring's dead slots are poison as well: zeros with priorities of
1e30 in the first run, bytes of 0xFF (NaN priorities) in the second. The result must not move, and the dead slots must keep
their bytes."""
import numpy as np
import pytest
import torch

import guard
import per_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 256                      # G2048_PER_SCAN_TILE (asserted below)
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
U8, I64, F32 = torch.uint8, torch.int64, torch.float32
RING = ("states", "next_states", "actions", "rewards", "dones", "priorities")


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge
    ge.ensure_built()
    pkg = ge.import_package()
    assert pkg._lib.PER_SCAN_TILE == TILE
    return pkg.ops


def twice(call):
    return {k: v.numpy() for k, v in guard.twice(DEV, call).items()}


def random_ring(rng, size):
    """`size` live transitions in logical order: (states, next_states, actions, rewards, dones, priorities)."""
    prio = np.exp(rng.normal(0.0, 1.5, size)).astype(np.float32)
    prio[rng.random(size) < 0.05] = np.float32(1e-5)
    return (rng.integers(0, 12, (size, 16)).astype(np.uint8), rng.integers(0, 12, (size, 16)).astype(np.uint8),
            rng.integers(0, 4, size).astype(np.uint8), rng.normal(0, 10, size).astype(np.float32), rng.integers(0, 2, size).astype(np.uint8), prio)


def physical(s, live, capacity, head):
    """The six ring arrays of `capacity` slots as guarded regions of the Set s, the live entries from `head` on, the dead slots
    poisoned with this run's byte (priorities: 1e30 or NaN). Returns (tensors, their initial values on the host)."""
    size = len(live[5])
    slots = (head + np.arange(size)) % capacity
    arrays, first = [], []
    for name, a in zip(RING, live):
        full = np.empty((capacity,) + a.shape[1:], a.dtype)
        full.view(np.uint8).fill(s.band)
        if name == "priorities" and s.band == 0:
            full.fill(1e30)
        full[slots] = a
        arrays.append(s.inp(name, full, 16 if a.ndim == 2 else None))
        first.append(full)
    return arrays, first


def dead_slots_kept(arrays, first, capacity, head, size):
    """One flag: every dead slot of every ring array still holds the bytes it was given."""
    dead = np.setdiff1d(np.arange(capacity), (head + np.arange(size)) % capacity)
    if len(dead) == 0:
        return torch.ones(1, dtype=torch.bool)
    idx = torch.from_numpy(dead).to(DEV)
    ok = [torch.equal(t.index_select(0, idx).contiguous().view(U8).cpu(), torch.from_numpy(np.ascontiguousarray(f[dead])).view(U8))
          for t, f in zip(arrays, first)]
    return torch.tensor([all(ok)])


def logical(arrays, capacity, head, size):
    order = ((torch.arange(size, device=DEV) + head) % capacity)
    return {name: t.index_select(0, order) for name, t in zip(RING, arrays)}


# ------------------------------------------------------------------------------------------------------------------- push --
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("size,head,m", [(0, 0, 1), (0, 7, 100), (70, 45, 1), (70, 45, 60), (70, 45, 100), (100, 99, 60)])
def test_per_push(ops, size, head, m, f64):
    """m in {1, 60, capacity} into a ring of 100 whose live entries cross its end; the workspace is exactly the stated size."""
    capacity = 100
    rng = np.random.default_rng(1000 * size + m)
    live = random_ring(rng, size)
    new = random_ring(rng, m)
    rewards_in = new[3].astype(np.float64) * 1.0000001 if f64 else new[3]
    flags = (new[4] | 0x02 | (5 << 3)).astype(np.uint8)             # as the step kernels write them: only bit 0 counts

    def call(s):
        arrays, first = physical(s, live, capacity, head)
        ws = s.out("workspace", ops.per_update_workspace_bytes(capacity), (), U8, 16)
        new_size, new_head = ops.per_push(*arrays, size, head, s.inp("boards", new[0], 16), s.inp("actions_in", new[2]),
                                          s.inp("rewards_in", rewards_in), s.inp("next_boards", new[1], 16), s.inp("flags", flags), workspace=ws)
        torch.cuda.synchronize()
        out = logical(arrays, capacity, new_head, new_size)
        out["dead_kept"] = dead_slots_kept(arrays, first, capacity, new_head, new_size)
        out["size_head"] = torch.tensor([new_size, new_head])
        return out
    got = twice(call)
    buf = R.Buffer(capacity, 0.6)
    buf.states, buf.next_states, buf.actions, buf.rewards, buf.dones, buf.priorities = live
    buf.push(new[0], new[2], rewards_in, new[1], new[4])
    assert got["dead_kept"].all() and got["size_head"][0] == len(buf) == min(size + m, capacity)
    assert got["size_head"][1] == (head + max(0, size + m - capacity)) % capacity
    for name, want in zip(RING, (buf.states, buf.next_states, buf.actions, buf.rewards, buf.dones, buf.priorities)):
        assert guard.same_bits(got[name], want), name


# ----------------------------------------------------------------------------------------------------------------- sample --
@pytest.mark.parametrize("head_kind", [0, 1])
@pytest.mark.parametrize("size", [1, TILE - 1, TILE, TILE + 1, 64 * TILE + 1])
def test_per_sample(ops, size, head_kind):
    """capacity = size + 5, the head at 0 or such that the live entries cross the ring's end, batch in {1, 255, 256, 257} where the
    size allows, want_probs on, a workspace of exactly g2048_per_sample_workspace(size, batch) bytes. The reference is
    tests/test_gpu_per.py's: the indices are searchsorted of the launch's own probs (the only draws left out being those within
    size * 2^-52 of a cdf entry), the probs the float64 formula's to 1e-5 of the largest, the gathered batch the ring's rows and
    per_ref's shaping; the weights are held to 8 x the float32 formula's own error against float64 (and one float32 ulp of 1)."""
    capacity = size + 5
    head = 0 if head_kind == 0 else capacity - min(2, size) if size > 1 else capacity - 1
    rng = np.random.default_rng(1000 * size + head_kind)
    live = random_ring(rng, size)
    st, nx, ac, rw, dn, prio = live
    alpha, beta = 0.6, 0.4
    drawn = left_out = 0
    for batch in (1, 255, 256, 257):
        if batch > size:
            continue
        u = rng.random(batch)
        u[0] = 0.0 if batch > 1 else u[0]
        u[-1] = 1.0 - 2.0 ** -30

        def call(s):
            arrays, first = physical(s, live, capacity, head)
            ws = s.out("workspace", ops.per_sample_workspace_bytes(size, batch), (), U8, 16)
            shapes = (("indices", (), I64, None), ("weights", (), F32, None), ("states", (16,), F32, 16), ("actions", (), I64, None),
                      ("rewards", (), F32, None), ("next_states", (16,), F32, 16), ("dones", (), F32, None), ("shaped", (), F32, None))
            out = {k: s.out("out_" + k, batch, tail, dtype, align) for k, tail, dtype, align in shapes}
            out["probs"] = s.out("out_probs", size, (), F32)
            r = ops.per_sample(*arrays, size, head, alpha, beta, batch, u=s.inp("u", u), workspace=ws, out=out)
            assert all(r[k] is out[k] for k in out)
            torch.cuda.synchronize()
            out = dict(out, dead_kept=dead_slots_kept(arrays, first, capacity, head, size))
            out.update({"ring_" + k: v for k, v in logical(arrays, capacity, head, size).items()})
            return out
        got = twice(call)
        assert got["dead_kept"].all()
        for name, a in zip(RING, live):
            assert guard.same_bits(got["ring_" + name], a), "sample modified the ring's %s" % name
        probs, idx = got["probs"], got["indices"]
        p64 = R.probs_f64(prio, alpha)
        assert (probs > 0).all() and np.abs(probs - p64).max() <= 1e-5 * p64.max()
        cdf = R.cdf_of(probs)
        near = R.near_cdf(cdf, u, size * 2.0 ** -52)
        differs = idx != R.search(cdf, u)
        assert not (differs & ~near).any(), (batch, np.flatnonzero(differs & ~near))
        assert (idx >= 0).all() and (idx < size).all()
        drawn, left_out = drawn + batch, left_out + int(near.sum())
        assert np.array_equal(got["states"], R.tiles_f32(st[idx])) and np.array_equal(got["next_states"], R.tiles_f32(nx[idx]))
        assert np.array_equal(got["actions"], ac[idx].astype(np.int64)) and guard.same_bits(got["rewards"], rw[idx])
        assert np.array_equal(got["dones"], dn[idx].astype(np.float32))
        assert guard.same_bits(got["shaped"], R.shaped_rewards(st[idx], nx[idx], rw[idx]))
        w64 = R.weights_f64(probs.astype(np.float64), idx, size, beta)
        ref_err = np.abs(R.weights_of(probs, idx, size, beta).astype(np.float64) - w64).max()
        err = np.abs(got["weights"].astype(np.float64) - w64).max()
        print("size %d batch %d: weights error %.3g, the float32 formula's own %.3g" % (size, batch, err, ref_err))
        assert err <= 8 * max(ref_err, 2.0 ** -23) and got["weights"].max() == np.float32(1.0)
    assert left_out <= 0.001 * drawn, (left_out, drawn)


# ------------------------------------------------------------------------------------------------------ update_priorities --
@pytest.mark.parametrize("n", SIZES)
def test_per_update_priorities(ops, n):
    """n indices -- out of range, negative and duplicated among them -- into a ring of 70 slots with 65 live ones across its end."""
    capacity, size = 70, 65
    head = capacity - 2
    rng = np.random.default_rng(n)
    live = random_ring(rng, size)
    indices = rng.integers(-5, size + 12, n).astype(np.int64)
    indices[rng.random(n) < 0.1] = 1 << 40
    indices[::7] = 3                                                # many duplicates of one slot: the latest wins
    td = rng.random(n).astype(np.float32) * 3
    td[rng.random(n) < 0.1] = 0.0

    def call(s):
        arrays, first = physical(s, live, capacity, head)
        ws = s.out("workspace", ops.per_update_workspace_bytes(capacity), (), U8, 16)
        ops.per_update_priorities(arrays[5], size, head, s.inp("indices", indices), s.inp("td", td), workspace=ws)
        torch.cuda.synchronize()
        out = logical(arrays, capacity, head, size)
        out["dead_kept"] = dead_slots_kept(arrays, first, capacity, head, size)
        return out
    got = twice(call)
    buf = R.Buffer(capacity, 0.6)
    buf.priorities = live[5].copy()
    buf.update_priorities(indices, td)
    assert got["dead_kept"].all() and guard.same_bits(got["priorities"], buf.priorities)
    for name, a in zip(RING[:5], live):
        assert guard.same_bits(got[name], a), name


# ---------------------------------------------------------------------------------------------------------------- shaping --
@pytest.mark.parametrize("n", SIZES)
def test_dqn_shape_rewards(ops, n):
    rng = np.random.default_rng(n + 7)
    st, nx, _, rw, _, _ = random_ring(rng, n)
    nx[::3] = np.maximum(nx[::3], st[::3])                          # some next states that reach a new maximum, some that do not
    got = twice(lambda s: {"out": ops.dqn_shape_rewards(s.inp("states", st, 16), s.inp("next_states", nx, 16), s.inp("rewards", rw),
                                                       out=s.out("out", n, (), F32))})
    assert guard.same_bits(got["out"], R.shaped_rewards(st, nx, rw))
