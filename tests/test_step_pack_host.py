"""g2048_step_pack / g2048_step_packed without a device: g2048_step_pack makes no HIP call, so every refusal and the accepted
case run on a CPU-only host. Pointer values are plain integers that nothing dereferences."""
import ctypes as C

import pytest

F64, AR, RAND, NOOP = 0x01, 0x02, 0x04, 0x08
P = 0x7f0000001000            # "device pointers": 16-byte aligned integers


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from g2048 import _lib
    return _lib


@pytest.fixture()
def block(L):
    buf = (C.c_uint64 * (L.STEP_CALL_BYTES // 8))()
    return buf, C.addressof(buf)


def pack(L, call, ptrs=None, seed=1, base=0, n=100, opts=0):
    p = [P, P + 0x1000, P + 0x2000, P + 0x3000, P + 0x4000, P + 0x5000] if ptrs is None else ptrs
    return L.lib().g2048_step_pack(*p, seed, base, n, opts, call)


def test_pack_accepts_and_packed_wants_the_magic_word(L, block):
    buf, call = block
    assert L.STEP_CALL_BYTES == 128
    zero = (C.c_uint64 * 16)()
    assert L.lib().g2048_step_packed(C.addressof(zero), 0, None) == -1 and b"g2048_step_pack" in L.lib().g2048_last_error()
    assert L.lib().g2048_step_packed(None, 0, None) == -1
    for opts in (0, F64, AR, F64 | AR, 1 << 8, 2 << 8, F64 | AR | (2 << 8)):
        assert pack(L, call, opts=opts) == 0, hex(opts)
        assert any(buf)
    # a refused pack leaves a block g2048_step_packed does not take
    assert pack(L, call, opts=0x80) == -1
    assert L.lib().g2048_step_packed(call, 0, None) == -1


def test_pack_rejects_what_step_rejects(L, block):
    _, call = block
    good = [P, P + 0x1000, P + 0x2000, P + 0x3000, P + 0x4000, P + 0x5000]
    for k in range(6):                                           # each null pointer
        bad = list(good)
        bad[k] = None
        assert pack(L, call, bad) == -1 and b"null pointer" in L.lib().g2048_last_error(), k
    assert pack(L, None) == -1                                   # no block to fill
    for k, off, opts in ((0, 8, 0), (2, 4, 0), (3, 2, 0), (4, 2, 0), (4, 4, F64)):       # boards in / out, score, f32 and f64 reward
        bad = list(good)
        bad[k] += off
        assert pack(L, call, bad, opts=opts) == -1 and b"align" in L.lib().g2048_last_error(), (k, off)
    assert pack(L, call, [P, P + 0x1000, P + 0x2000, P + 0x3000, P + 0x4004, P + 0x5000]) == 0      # an f32 reward on a 4-byte boundary is fine
    assert pack(L, call, opts=0x80) == -1 and b"opts" in L.lib().g2048_last_error()
    assert pack(L, call, opts=0x1000) == -1 and b"opts" in L.lib().g2048_last_error()
    assert pack(L, call, opts=3 << 8) == -1 and b"tune 3" in L.lib().g2048_last_error()


def test_pack_refuses_what_is_not_one_plain_launch(L, block):
    _, call = block
    assert pack(L, call, opts=RAND) == -1 and b"RANDOM_ACTIONS" in L.lib().g2048_last_error()
    assert pack(L, call, [P, None, P + 0x2000, P + 0x3000, P + 0x4000, P + 0x5000], opts=RAND) == -1
    assert pack(L, call, opts=NOOP) == -1 and b"NOOP_ACTIONS" in L.lib().g2048_last_error()
    assert pack(L, call, base=2**32 - 5, n=10) == -1 and b"2^32" in L.lib().g2048_last_error()
    assert pack(L, call, base=2**32 - 5, n=5) == 0               # ends exactly at the multiple: one launch
    assert pack(L, call, base=(7 << 32) + 2**32 - 5, n=6) == -1
    assert pack(L, call, base=(7 << 32) + 2**32 - 5, n=5) == 0
