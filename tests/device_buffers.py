"""Guard-banded buffers for the tests of where an entry point reads and writes in its caller's memory.

A buffer handed to the library is the INTERIOR of one larger allocation whose every word -- both bands and, until the
test fills it, the interior -- holds a position-dependent sentinel in [p, 2^64): 0xFFFFFFFF00000001 + (i & 0xFFFF) for the
word at allocation index i.  No canonical field element equals a sentinel, so
  * a word the library wrote where it should not have is visible (the bands, stride padding, anything behind an output),
  * a sentinel the library READ by mistake shows up in its result (a leaf of at most four words is its own digest; a
    reduced sentinel is never the value the reference was given),
and neighbouring sentinels differ, so a block copied from the wrong offset does not pass for the right one.

Bands are at least 4096 words.  `before` may be odd: include/p25.h promises its callers no alignment beyond that of a
uint64_t (uint32_t for status arrays), and an interior that starts an odd number of words into a torch allocation is
aligned to exactly that and no more.

Device buffers are built the way the suite builds every device buffer: numpy uint64 -> .view(np.int64) ->
torch.from_numpy -> .to(device)."""
import numpy as np

P = 0xFFFFFFFF00000001
MIN_BAND = 4096
SENTINEL32 = 0xA5A5A5A5


def sentinels(n, start=0):
    """Sentinel words of allocation indices start .. start + n."""
    return np.uint64(P) + ((np.arange(n, dtype=np.uint64) + np.uint64(start)) & np.uint64(0xFFFF))


def _first_bad(got, want):
    bad = np.nonzero(got != want)[0]
    return f"{bad.size} words differ, first at {bad[:8].tolist()}: got {[hex(int(v)) for v in got[bad[:4]]]}"


class _BandedBase:
    """The bookkeeping both memory kinds share.  `expect` mirrors what the test itself put into the allocation."""

    def _init_layout(self, n_words, before, after, fill):
        assert before >= MIN_BAND and after >= MIN_BAND and n_words >= 0
        self.n, self.before, self.after = int(n_words), int(before), int(after)
        self.expect = fill(self.before + self.n + self.after)
        self._sentinel = self.expect.copy()

    def _whole(self):
        raise NotImplementedError

    def get(self):
        """The interior, as a numpy copy."""
        return self._whole()[self.before:self.before + self.n].copy()

    def assert_bands_intact(self):
        w = self._whole()
        lo, hi = w[:self.before], w[self.before + self.n:]
        assert (lo == self._sentinel[:self.before]).all(), "band BEFORE the buffer: " + _first_bad(lo, self._sentinel[:self.before])
        assert (hi == self._sentinel[self.before + self.n:]).all(), \
            "band BEHIND the buffer: " + _first_bad(hi, self._sentinel[self.before + self.n:])

    def assert_untouched(self, index):
        """Interior words that must never be written (stride padding): they still hold their sentinels."""
        idx = np.asarray(index, dtype=np.int64)
        if idx.size == 0:
            return
        assert idx.min() >= 0 and idx.max() < self.n
        got, want = self.get()[idx], self._sentinel[self.before + idx]
        assert (got == want).all(), "padding: " + _first_bad(got, want)

    def assert_unchanged(self):
        """Bands and interior are bit for bit what the test put there (inputs; outputs of a refused call)."""
        w = self._whole()
        assert (w == self.expect).all(), "buffer changed: " + _first_bad(w, self.expect)


class Banded(_BandedBase):
    """n_words 64-bit words of device memory inside one torch allocation of before + n_words + after."""
    np_dtype, view_dtype, itemsize = np.uint64, np.int64, 8

    def __init__(self, n_words, before=MIN_BAND, after=MIN_BAND, device=None):
        import torch
        self._init_layout(n_words, before, after, self._fill)
        self.device = device if device is not None else torch.device("cuda", 0)
        self._t = torch.from_numpy(self.expect.view(self.view_dtype).copy()).to(self.device)
        self._pinned = []

    @staticmethod
    def _fill(total):
        return sentinels(total)

    @property
    def ptr(self):
        """Device address of the interior."""
        return self._t.data_ptr() + self.itemsize * self.before

    def _whole(self):
        return self._t.cpu().numpy().view(self.np_dtype)

    def _host(self, array, offset):
        a = np.ascontiguousarray(array, dtype=self.np_dtype).ravel()
        assert 0 <= offset and offset + a.size <= self.n
        self.expect[self.before + offset:self.before + offset + a.size] = a
        return a

    def set(self, array, offset=0):
        """Copy `array` into the interior at word `offset` (blocking, on the current stream)."""
        import torch
        a = self._host(array, offset)
        if a.size:
            lo = self.before + offset
            self._t[lo:lo + a.size] = torch.from_numpy(a.view(self.view_dtype)).to(self.device)

    def set_async(self, array, stream, offset=0, before_enqueue=None):
        """The same as a non-blocking copy from pinned host memory ENQUEUED ON `stream` (a torch.cuda.Stream): until that
        stream reaches the copy the interior still holds sentinels.  before_enqueue() is called once the pinned copy
        exists, right before the enqueue (the caller's chance to put work on the stream in front of it)."""
        import torch
        a = self._host(array, offset)
        pinned = torch.from_numpy(a.view(self.view_dtype).copy()).pin_memory() if a.size else None
        self._pinned.append(pinned)                          # must outlive the copy
        if before_enqueue is not None:
            before_enqueue()
        if a.size:
            lo = self.before + offset
            with torch.cuda.stream(stream):
                self._t[lo:lo + a.size].copy_(pinned, non_blocking=True)


class Banded32(Banded):
    """The 32-bit variant for status arrays: every word 0xA5A5A5A5 until written."""
    np_dtype, view_dtype, itemsize = np.uint32, np.int32, 4

    @staticmethod
    def _fill(total):
        return np.full(total, SENTINEL32, dtype=np.uint32)


class BandedHost(_BandedBase):
    """The same in host memory, for host outputs: `array` is the interior (a view: pass it to ctypes as it is)."""

    def __init__(self, n_words, before=MIN_BAND, after=MIN_BAND, dtype=np.uint64):
        if np.dtype(dtype) == np.uint64:
            fill = sentinels
        else:
            assert np.dtype(dtype).itemsize == 4
            fill = lambda total: np.full(total, SENTINEL32, dtype=dtype)   # noqa: E731
        self._init_layout(n_words, before, after, fill)
        self._a = self.expect.copy()
        self.array = self._a[self.before:self.before + self.n]

    @property
    def ptr(self):
        import ctypes as C
        return C.c_void_p(self._a.ctypes.data + self._a.itemsize * self.before)

    def _whole(self):
        return self._a

    def set(self, array, offset=0):
        a = np.ascontiguousarray(array, dtype=self._a.dtype).ravel()
        assert 0 <= offset and offset + a.size <= self.n
        self.array[offset:offset + a.size] = a
        self.expect[self.before + offset:self.before + offset + a.size] = a


def banded_host(n_words, before=MIN_BAND, after=MIN_BAND, dtype=np.uint64):
    return BandedHost(n_words, before, after, dtype)


def strided_rows(rows, width, stride):
    """(data index, padding index) of `rows` rows of `width` words laid `stride` words apart in a buffer of
    (rows - 1) * stride + width ... rows * stride words: index arrays into the interior."""
    base = np.arange(rows, dtype=np.int64)[:, None] * stride
    data = (base + np.arange(width, dtype=np.int64)[None, :]).ravel()
    pad = (base + np.arange(width, stride, dtype=np.int64)[None, :]).ravel()
    return data, pad
