"""Guard bands (tests/guard.py) round the arrays of the rollout's entry points (csrc/g2048_rollout.hip): the fused rollout step with
all nine outputs, the minibatch gather, and the shaping chain through the raw entry points, so that the scan's workspace (at
exactly the stated size) and the seen-states table can be guarded. The protocol is tests/test_gpu_bounds.py's: two runs from
identical data, bands of 0x00 and then of 0xFF, every band intact, the results equal bit for bit and equal to the reference of
tests/test_gpu_rollout.py (the CPU oracle, its sequential remember(), and that file's feistel_indices).

Where a key lands in the seen-states table depends on which lane reaches a contended slot first, so a table is compared as the
sorted set of its (key, first index) entries and the slot numbers by what they point at."""
import numpy as np
import pytest
import torch

import guard
from test_gpu_rollout import feistel_indices

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
SCAN_TILE = 4096                # transitions per block of g2048_shaping_scan
U8, I32, I64, F32, F64 = torch.uint8, torch.int32, torch.int64, torch.float32, torch.float64


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
    return guard.twice(DEV, call)


# ------------------------------------------------------------------------------------------------------------ rollout step --
@pytest.mark.parametrize("obs_dtype,reward_dtype,give_mask", [(torch.float32, torch.float32, True), (torch.float16, torch.float64, False),
                                                              (torch.bfloat16, torch.float32, True)])
@pytest.mark.parametrize("n", SIZES)
def test_rollout_step_all_outputs(ops, oracle, n, obs_dtype, reward_dtype, give_mask):
    seed, t, base = 0xFEED, 47, 123456789
    hb = oracle.synth_boards(n, seed=5, id_base=n, p_empty=0.2, max_code=6)
    k = n // 3
    hb[:k] = oracle.synth_boards(k, seed=6, p_empty=0.0, max_code=3)              # nearly dead boards: auto-resets happen
    probs = np.random.default_rng(n).dirichlet(np.ones(4), n).astype(np.float32)
    mask = oracle.valid_moves_batch(hb)
    hs = (np.arange(n) * 4).astype(np.int32)
    counter = np.array([40], np.int64)

    def call(s):
        sc = s.inp("scores", hs)
        o = {"out": s.out("out", n, (16,), U8, 16), "actions": s.out("actions", n), "prob": s.out("prob", n, (), F32),
             "reward": s.out("reward", n, (), reward_dtype), "flags": s.out("flags", n), "obs_next": s.out("obs_next", n, (16,), obs_dtype, 16),
             "mask_next": s.out("mask_next", n), "next_boards": s.out("next_boards", n, (16,), U8, 16),
             "state_maxcode": s.out("state_maxcode", n), "scores": sc}
        ops.rollout_step(s.inp("boards", hb, 16), s.inp("probs", probs, 16), sc, seed, t - 40, base, mask=s.inp("mask", mask) if give_mask else None,
                         out=o["out"], actions=o["actions"], prob=o["prob"], reward=o["reward"], flags=o["flags"], obs_next=o["obs_next"],
                         mask_next=o["mask_next"], next_boards=o["next_boards"], state_maxcode=o["state_maxcode"], auto_reset=True,
                         step_counter=s.inp("step_counter", counter))
        return o
    got = twice(call)
    a, pa = oracle.sample_batch(probs, mask, seed=seed, step_index=t, id_base=base)
    b, sc, rw, fl = oracle.step_batch(hb, a, hs.astype(np.uint32), seed=seed, step_index=t, id_base=base, opts=1)
    nb, _, _, _ = oracle.step_batch(hb, a, hs.astype(np.uint32), seed=seed, step_index=t, id_base=base, opts=0)
    assert np.array_equal(got["actions"].numpy(), a) and guard.same_bits(got["prob"], pa)
    assert np.array_equal(got["out"].numpy(), b) and np.array_equal(got["scores"].numpy().astype(np.uint32), sc)
    assert np.array_equal(got["flags"].numpy(), fl) and guard.same_bits(got["reward"], rw.astype(np.float64 if reward_dtype == F64 else np.float32))
    assert guard.same_bits(got["obs_next"], torch.from_numpy(oracle.obs_batch(b)).to(obs_dtype))
    assert np.array_equal(got["mask_next"].numpy(), oracle.valid_moves_batch(b))
    assert np.array_equal(got["next_boards"].numpy(), nb) and np.array_equal(got["state_maxcode"].numpy(), hb.max(axis=1))


# --------------------------------------------------------------------------------------------------------------- minibatch --
@pytest.mark.parametrize("obs_dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("n", [1, 255, 5000])
def test_minibatch_gather(ops, oracle, n, obs_dtype):
    """The seven outputs, the indices among them, for batches of 1, 64, 257 and one larger than the buffer (then the whole buffer)."""
    rng = np.random.default_rng(n)
    hb = oracle.synth_boards(n, seed=77, id_base=n)
    nxt = oracle.synth_boards(n, seed=78, id_base=n)
    obs = torch.from_numpy(oracle.obs_batch(hb)).to(obs_dtype)
    acts = oracle.synth_actions(n, seed=77)
    logp = rng.normal(size=n).astype(np.float32)
    rew = rng.normal(size=n) * 1e3
    flags = ((rng.random(n) < 0.1).astype(np.uint8) | 0x02 | (5 << 3)).astype(np.uint8)      # as a step writes them: bit 0 = done
    seed, sample_index = 5, 3
    k0, k1 = oracle.rng_keys(seed, 9, sample_index)                    # DOM_MINIBATCH
    for asked in (1, 64, 257, n + 3):
        batch = min(asked, n)

        def call(s):
            out = {"states": s.out("states", batch, (16,), F32, 16), "actions": s.out("actions", batch, (), I64),
                   "old_log_probs": s.out("old_log_probs", batch, (), F32), "rewards": s.out("rewards", batch, (), F32),
                   "next_states": s.out("next_states", batch, (16,), F32, 16), "dones": s.out("dones", batch, (), F32),
                   "indices": s.out("indices", batch, (), I64)}
            r = ops.minibatch_gather(s.inp("obs", obs, 16), s.inp("acts", acts), s.inp("logp", logp), s.inp("rew", rew), s.inp("nxt", nxt, 16),
                                     s.inp("flags", flags), asked, seed, sample_index, out=out)
            assert r is out
            return out
        got = {k: v.numpy() for k, v in twice(call).items()}
        idx = got["indices"]
        assert np.array_equal(idx, feistel_indices(batch, n, k0, k1)) and len(np.unique(idx)) == batch
        assert guard.same_bits(got["states"], obs[idx].float()) and np.array_equal(got["actions"], acts[idx].astype(np.int64))
        assert guard.same_bits(got["old_log_probs"], logp[idx]) and guard.same_bits(got["rewards"], rew[idx].astype(np.float32))
        assert guard.same_bits(got["next_states"], oracle.obs_batch(nxt[idx])) and np.array_equal(got["dones"], (flags[idx] & 1).astype(np.float32))


# ----------------------------------------------------------------------------------------------------------- shaping chain --
def table_entries(table):
    """The full slots of a seen-states table as sorted rows (key_lo, key_hi, first index), and whether every other slot is still
    all zero."""
    t = table.detach().cpu().contiguous().view(I64).view(-1, 4).numpy()
    full = (t[:, 3] & 0xFFFFFFFF) == 2
    rows = t[full][:, :3]
    rows = rows[np.lexsort(rows.T[::-1])] if len(rows) else rows
    return torch.from_numpy(np.ascontiguousarray(rows)), bool((t[~full] == 0).all()) and bool((t[full][:, 3] == 2).all())


def keys_of(boards):
    """The two 64-bit halves of each board, as a slot holds them."""
    return np.ascontiguousarray(boards).view(np.int64).reshape(-1, 2)


def transitions(oracle, n, distinct):
    """n ordered transitions over a pool of `distinct` boards whose largest code grows with the pool index, drawn from a prefix of
    the pool that grows along the batch: boards repeat, and the running maximum moves at many places."""
    rng = np.random.default_rng(n)
    pool = oracle.synth_boards(distinct, seed=77, id_base=n)
    pool[:, 0] = np.maximum(pool[:, 0], 1)
    pool = np.minimum(pool, np.minimum(17, 1 + np.arange(distinct) * 16 // distinct).astype(np.uint8)[:, None])
    nxt = pool[rng.integers(0, 1 + np.arange(n) * distinct // n)]
    st = pool[rng.integers(0, distinct, n)]
    return st, nxt, rng.normal(size=n)


@pytest.mark.parametrize("n", SIZES + [SCAN_TILE + 1])
def test_shaping_chain(ops, oracle, n):
    """g2048_shaping_scan (workspace of exactly g2048_shaping_scan_workspace(n) bytes) -> g2048_seen_insert (2^10 slots) ->
    g2048_shaping_apply == the oracle's sequential remember()."""
    from g2048 import _lib as L
    st, nxt, rin = transitions(oracle, n, min(n, 300))
    flags = (nxt.max(axis=1) << 3).astype(np.uint8)
    state_max = st.max(axis=1)
    log2 = 10

    def call(s):
        fl, nb = s.inp("flags", flags, 16), s.inp("next_boards", nxt, 16)
        prev = s.out("prev_highest", n, (), U8, 16)
        highest = s.inp("highest", np.array([1], np.int32))
        ws = s.out("workspace", int(L.lib().g2048_shaping_scan_workspace(n)), (), U8, 16)
        raw("g2048_shaping_scan", fl, prev, highest, ws, n)
        table = s.inp("table", np.zeros((1 << log2, L.SEEN_SLOT_BYTES), np.uint8), 16)
        count, overflow = s.inp("count", np.zeros(1, np.int64)), s.inp("overflow", np.zeros(1, np.int32))
        slots = s.out("slots", n, (), I32)
        raw("g2048_seen_insert", nb, 0, table, log2, count, overflow, slots, n)
        shaped, novel = s.out("shaped", n, (), F64), s.out("novel", n)
        raw("g2048_shaping_apply", nb, s.inp("state_max", state_max), fl, s.inp("env_reward", rin), prev, table, slots, 0, shaped, novel, n)
        torch.cuda.synchronize()
        entries, clean = table_entries(table)
        at = table.view(I64).view(-1, 4)[slots.long()][:, :2].cpu().numpy()            # what each transition's slot holds: its own board
        return {"prev_highest": prev, "highest": highest, "count": count, "overflow": overflow, "shaped": shaped, "novel": novel,
                "entries": entries, "table_ok": torch.tensor([clean and np.array_equal(at, keys_of(nxt))])}
    got = {k: v.numpy() for k, v in twice(call).items()}
    want, novel = oracle.Remember().batch(st, nxt, rin)
    codes = (flags >> 3).astype(np.int64)
    assert np.array_equal(got["prev_highest"], np.maximum.accumulate(np.concatenate([[1], codes]))[:-1])
    assert got["highest"][0] == max(1, codes.max()) and got["overflow"][0] == 0 and got["table_ok"].all()
    assert guard.same_bits(got["shaped"], want) and np.array_equal(got["novel"].astype(bool), novel)
    uniq, first = np.unique(keys_of(nxt), axis=0, return_index=True)
    assert got["count"][0] == len(uniq) == novel.sum()
    rows = np.concatenate([uniq, first[:, None]], axis=1)
    assert np.array_equal(got["entries"], rows[np.lexsort(rows.T[::-1])])


@pytest.mark.parametrize("n", [1, 16, 17, 64, 257])
def test_seen_insert_into_the_smallest_table(ops, oracle, n):
    """2^4 slots and n distinct boards: up to 16 of them fit; a larger batch overflows. The overflow flag is the result then, and
    the bands round the table, the count and the slot numbers survive it."""
    from g2048 import _lib as L
    boards = oracle.synth_boards(n, seed=31, id_base=n, p_empty=0.3, max_code=11)
    assert len(np.unique(keys_of(boards), axis=0)) == n

    def call(s):
        table = s.inp("table", np.zeros((16, L.SEEN_SLOT_BYTES), np.uint8), 16)
        count, overflow = s.inp("count", np.zeros(1, np.int64)), s.inp("overflow", np.zeros(1, np.int32))
        slots = s.out("slots", n, (), I32)
        raw("g2048_seen_insert", s.inp("boards", boards, 16), 100, table, 4, count, overflow, slots, n)
        torch.cuda.synchronize()
        entries, clean = table_entries(table)
        stored = slots.cpu().numpy() != -1
        at = table.view(I64).view(-1, 4)[slots.long().clamp(min=0)][:, :3].cpu().numpy()
        own = np.concatenate([keys_of(boards), 100 + np.arange(n)[:, None]], axis=1)
        ok = clean and np.array_equal(at[stored], own[stored]) and int(stored.sum()) == len(entries)
        out = {"count": count, "overflow": overflow, "table_ok": torch.tensor([ok]), "stored": torch.tensor([int(stored.sum())])}
        if n <= 16:
            out["entries"] = entries            # (which boards a table that is too small keeps depends on who came first)
        return out
    got = {k: v.numpy() for k, v in twice(call).items()}
    assert got["table_ok"].all() and got["count"][0] == got["stored"][0] == min(n, 16)
    assert (got["overflow"][0] != 0) == (n > 16)
    if n <= 16:
        rows = np.concatenate([keys_of(boards), 100 + np.arange(n)[:, None]], axis=1)
        assert np.array_equal(got["entries"], rows[np.lexsort(rows.T[::-1])])


@pytest.mark.parametrize("n", [1, 9, 16])
def test_seen_rehash(ops, oracle, n):
    """2^4 -> 2^6 slots: every (key, first index) of the old table is in the new one, nothing else is, the old table is only read."""
    from g2048 import _lib as L
    boards = oracle.synth_boards(n, seed=32, id_base=n, p_empty=0.3, max_code=11)

    def call(s):
        old = s.inp("old_table", np.zeros((16, L.SEEN_SLOT_BYTES), np.uint8), 16)
        count, overflow = s.inp("count", np.zeros(1, np.int64)), s.inp("overflow", np.zeros(1, np.int32))
        raw("g2048_seen_insert", s.inp("boards", boards, 16), 7, old, 4, count, overflow, s.out("slots", n, (), I32), n)
        torch.cuda.synchronize()
        before = old.clone()
        new = s.inp("new_table", np.zeros((64, L.SEEN_SLOT_BYTES), np.uint8), 16)
        raw("g2048_seen_rehash", old, 4, new, 6, overflow)
        torch.cuda.synchronize()
        entries, clean = table_entries(new)
        return {"entries": entries, "overflow": overflow, "table_ok": torch.tensor([clean and torch.equal(before, old)]),
                "old_entries": table_entries(old)[0]}
    got = {k: v.numpy() for k, v in twice(call).items()}
    rows = np.concatenate([keys_of(boards), 7 + np.arange(n)[:, None]], axis=1)
    rows = rows[np.lexsort(rows.T[::-1])]
    assert got["table_ok"].all() and got["overflow"][0] == 0
    assert np.array_equal(got["entries"], rows) and np.array_equal(got["old_entries"], rows)
