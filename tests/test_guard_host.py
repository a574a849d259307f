"""tests/guard.py on CPU tensors: the layout it promises (band sizes, the data's alignment and no higher one), and the stated
outcome of check() for an untouched region, a byte changed before the data and a byte changed after it."""
import re

import numpy as np
import pytest
import torch

import guard

CASES = [(5, (16,), torch.uint8, 16), (7, (), torch.uint8, None), (3, (), torch.float32, None), (9, (4,), torch.float32, 16),
         (4, (16,), torch.float16, 8), (2, (8,), torch.int32, 16), (6, (), torch.float64, None), (1, (80,), torch.uint8, 16),
         (0, (16,), torch.uint8, 16), (11, (), torch.int64, None), (100, (), torch.uint8, 64)]


@pytest.mark.parametrize("rows,tail,dtype,align", CASES)
def test_layout(rows, tail, dtype, align):
    r = guard.Region(rows, tail, dtype=dtype, align=align)
    esize = torch.empty((), dtype=dtype).element_size()
    a = esize if align is None else align
    assert r.view.shape == (rows,) + tuple(tail) and r.view.dtype == dtype and r.view.is_contiguous()
    assert r.address % a == 0 and r.address % (2 * a) != 0 and (rows == 0 or r.view.data_ptr() == r.address)
    assert r.address == r.raw.data_ptr() + r.lo and r.hi - r.lo == r.view.numel() * esize
    band = max(1024 * r.row_bytes, 4096)
    assert r.lo >= band and r.raw.numel() - r.hi >= band
    r.view.fill_(1)                                     # writing all of the data touches no band
    r.check("x")
    assert r.changed() is None


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_bands_are_what_was_asked_for(byte):
    r = guard.Region(3, (4,), dtype=torch.float32, align=16).fill_bands(byte)
    assert bool((r.raw[:r.lo] == byte).all()) and bool((r.raw[r.hi:] == byte).all())
    f = r.raw[r.hi:r.hi + 16].view(torch.float32)       # the row past the end, as the kernel would read it
    assert bool(torch.isnan(f).all()) if byte == 0xFF else bool((f == 0).all())
    i = guard.Region(3, (), dtype=torch.int64).fill_bands(0xFF)
    assert int(i.raw[i.hi:i.hi + 8].view(torch.int64)[0]) == -1


def _message(r, name):
    with pytest.raises(AssertionError) as e:
        r.check(name)
    return str(e.value)


@pytest.mark.parametrize("byte", [0x00, 0xFF])
@pytest.mark.parametrize("offset", [0, 1, 15, 4095])
def test_a_byte_changed_after_the_data(byte, offset):
    r = guard.Region(5, (16,), dtype=torch.uint8, align=16).fill_bands(byte)
    r.raw[r.hi + offset] = 0x11
    r.raw[r.hi + offset + 40] = 0x12                    # a later one: the first is reported
    msg = _message(r, "masks")
    assert r.changed() == ("after", offset, 2)
    assert "masks" in msg and "after" in msg and "before" not in msg and re.search(r"offset %d \(" % offset, msg)


@pytest.mark.parametrize("byte", [0x00, 0xFF])
@pytest.mark.parametrize("offset", [-1, -16, -4096])
def test_a_byte_changed_before_the_data(byte, offset):
    r = guard.Region(5, (), dtype=torch.float32).fill_bands(byte)
    r.raw[r.lo + offset] = 0x11
    msg = _message(r, "reward")
    assert r.changed() == ("before", offset, 1)
    assert "reward" in msg and "before" in msg and "after" not in msg and re.search(r"offset %d \(" % offset, msg)


def test_a_whole_row_stored_past_the_end():
    """What part 3 of the GPU file provokes: n + 1 rows stored into a region of n."""
    r = guard.Region(7, (16,), dtype=torch.float32, align=16).fill_bands(0xFF)
    r.raw[r.hi:r.hi + 64].view(torch.float32).fill_(0.5)
    assert r.changed() == ("after", 0, 64)
    assert "offset 0 " in _message(r, "obs")


def test_refilling_the_bands_moves_the_expectation():
    r = guard.Region(2, (16,), dtype=torch.uint8, align=16)
    r.check("x")
    r.fill_bands(0xFF)
    r.check("x")
    r.raw[0] = 0
    assert r.changed() == ("before", -r.lo, 1)


def test_of_copies_and_bits_compare_payloads():
    a = np.arange(48, dtype=np.uint8).reshape(3, 16)
    r = guard.Region.of(a, align=16)
    assert np.array_equal(r.view.numpy(), a) and r.view.data_ptr() % 32 == 16
    x = torch.tensor([0.0, float("nan")], dtype=torch.float32)
    y = x.clone()
    assert guard.same_bits(x, y)
    y.view(torch.int32)[1] ^= 1                         # another NaN
    assert not guard.same_bits(x, y)
    assert not guard.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))


def test_twice_checks_bands_and_equality():
    def good(s):
        src = s.inp("src", np.arange(10, dtype=np.float32))
        dst = s.out("dst", 10, (), torch.float32)
        dst.copy_(src * 2)
        return {"dst": dst}
    assert np.array_equal(guard.twice("cpu", good)["dst"].numpy(), np.arange(10, dtype=np.float32) * 2)

    def reads_the_band(s):                              # the result depends on what lies past the input
        src = s.inp("src", np.arange(10, dtype=np.float32))
        dst = s.out("dst", 10, (), torch.float32)
        r = s.regions["src"]
        dst.copy_(r.raw[r.lo + 4:r.hi + 4].view(torch.float32))
        return {"dst": dst}
    with pytest.raises(AssertionError, match="dst differs"):
        guard.twice("cpu", reads_the_band)

    def writes_nothing(s):                              # caught as a difference: the prefill is not the same in the two runs
        return {"dst": s.out("dst", 10, (), torch.float32)}
    with pytest.raises(AssertionError, match="dst differs"):
        guard.twice("cpu", writes_nothing)

    def overruns(s):
        dst = s.out("dst", 10, (), torch.float32)
        r = s.regions["dst"]
        r.raw[r.lo:r.hi + 4].view(torch.float32).fill_(1.0)
        return {"dst": dst}
    with pytest.raises(AssertionError, match="dst: the band after"):
        guard.twice("cpu", overruns)
