"""Guard bands round the arrays a test hands to the library: the only evidence, where no memory checker may run, that a kernel
stays inside what it was given (writes) and that nothing outside reaches a result (reads).

A `Region` is ONE allocation: a band, the data, a band. Each band is at least 1,024 rows of the array's row size and at least
4 KiB -- more than any block tile of the kernels can overrun -- so an overrun that a test catches is a store into memory the
test owns, never a fault. The data starts at exactly the alignment asked for and at no higher power of two: the byte before
it is then one that a wider aligned store would reach.

    r = guard.Region(n, (16,), dtype=torch.uint8, device=DEV, align=16)
    r.fill_bands(0xFF)              # NaN for float arrays, an index far out of range for integer arrays
    kernel(r.view.data_ptr(), ...)
    r.check("boards_out")           # AssertionError: which array, which band, the offset of the first changed byte

For an input the same class is used: its bands are then poison that must not be read. `Set` and `twice` are the two-run
protocol of tests/test_gpu_bounds*.py: the same call from identical data with bands of 0x00 and of 0xFF (outputs prefilled
differently), every band intact after each run and the outputs of both runs equal bit for bit."""
import numpy as np
import torch

BAND_ROWS = 1024
BAND_MIN_BYTES = 4096
RUNS = ((0x00, 0x3C), (0xFF, 0xC3))         # (band byte, byte the overwritten arrays are prefilled with) of the two runs


def _esize(dtype):
    return torch.empty((), dtype=dtype).element_size()


class Region:
    def __init__(self, rows, tail=(), dtype=torch.uint8, device="cpu", align=None):
        self.rows, self.tail, self.dtype = int(rows), tuple(int(t) for t in tail), dtype
        esize = _esize(dtype)
        self.align = esize if align is None else int(align)
        if self.align < esize or self.align & (self.align - 1):
            raise ValueError("guard: align must be a power of two, at least the element size")
        self.row_bytes = esize * int(np.prod(self.tail, dtype=np.int64)) if self.tail else esize
        self.nbytes = self.rows * self.row_bytes
        band = max(BAND_ROWS * self.row_bytes, BAND_MIN_BYTES)
        self.raw = torch.empty(band + self.nbytes + band + 2 * self.align, dtype=torch.uint8, device=device)
        base = self.raw.data_ptr()
        # the first offset past the band at which the address is `align` modulo 2 * align
        self.lo = band + (self.align - (base + band)) % (2 * self.align)
        self.hi = self.lo + self.nbytes
        self.address = base + self.lo           # (an empty view need not say where it starts)
        self.view = self.raw[self.lo:self.hi].view(dtype).view((self.rows,) + self.tail)
        assert (base + self.lo) % (2 * self.align) == self.align and self.raw.numel() - self.hi >= band
        self.byte = None
        self.fill_bands(0x00)

    @classmethod
    def of(cls, data, device=None, align=None):
        """A region that holds a copy of `data` (a tensor or an array)."""
        t = torch.as_tensor(np.ascontiguousarray(data)) if not isinstance(data, torch.Tensor) else data
        r = cls(t.shape[0], t.shape[1:], t.dtype, t.device if device is None else device, align)
        r.view.copy_(t)
        return r

    def fill_bands(self, byte):
        self.byte = int(byte) & 0xFF
        self.raw[:self.lo].fill_(self.byte)
        self.raw[self.hi:].fill_(self.byte)
        return self

    def fill_data(self, byte):
        self.raw[self.lo:self.hi].fill_(int(byte) & 0xFF)
        return self

    def changed(self):
        """None, or (band, offset, count): the band "before" or "after", the offset of its first changed byte -- relative to the
        data's first byte for the band before (so negative), to the first byte past the data for the band after -- and the
        number of changed bytes in that band."""
        for band, part, origin in (("before", self.raw[:self.lo], self.lo), ("after", self.raw[self.hi:], 0)):
            bad = part != self.byte
            if bool(bad.any()):
                first = int(torch.nonzero(bad)[0, 0])
                return band, first - origin, int(bad.sum())
        return None

    def check(self, name="array"):
        c = self.changed()
        if c is not None:
            band, offset, count = c
            raise AssertionError("%s: the band %s the data changed: first changed byte at offset %d (relative to the %s), %d bytes "
                                 "in all; the data are %d rows of %d bytes" % (
                                     name, band, offset, "data's start" if band == "before" else "data's end", count, self.rows,
                                     self.row_bytes))


def bits(t):
    """A tensor's bytes as integers, so that NaN payloads and signed zeros count in a comparison."""
    if isinstance(t, np.ndarray):
        t = torch.as_tensor(np.ascontiguousarray(t))
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bool:
        return t.to(torch.uint8)
    if not t.dtype.is_floating_point:
        return t
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a, b))


class Set:
    """The regions of one call. inp(): an array the call reads, or updates in place, holding a copy of `data`; out(): an array the
    call overwrites, prefilled with this run's byte. All bands hold this run's band byte; check() looks at every one of them,
    the inputs' too (nothing may write there either)."""

    def __init__(self, band, prefill, device):
        self.band, self.prefill, self.device = band, prefill, device
        self.regions = {}

    def _add(self, name, r):
        assert name not in self.regions, name
        self.regions[name] = r.fill_bands(self.band)
        return r.view

    def inp(self, name, data, align=None):
        return self._add(name, Region.of(data, self.device, align))

    def out(self, name, rows, tail=(), dtype=torch.uint8, align=None):
        return self._add(name, Region(rows, tail, dtype, self.device, align).fill_data(self.prefill))

    def check(self):
        for name, r in self.regions.items():
            r.check(name)


def twice(device, call):
    """call(S) -> dict of result tensors, made with a fresh Set for each of the two RUNS. Every band of every region is intact
    after each run and the two runs' results are equal bit for bit. Returns the first run's results (on the host)."""
    results = []
    for band, prefill in RUNS:
        s = Set(band, prefill, device)
        outs = call(s)
        if torch.device(device).type == "cuda":
            torch.cuda.synchronize()
        s.check()
        results.append({k: v.detach().cpu().clone() for k, v in outs.items()})
    for k in results[0]:
        assert same_bits(results[0][k], results[1][k]), "%s differs between the run with bands of 0x00 and the run with bands of 0xFF" % k
    return results[0]
