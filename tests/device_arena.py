"""A guard-banded device arena: what else did a device call touch?

One arena is one kzg_dev_alloc allocation whose host image is a numpy byte array filled with seeded pseudo-random bytes.
region() reserves a sub-range for one operand: an input's values are written into the image, an output keeps the fill.  Every
region has GUARD_ROWS rows of fill before and after it (one row more than the largest tile of the library, 2048), the gaps
between the columns of a strided region are fill as well, and every region starts at an odd multiple of 32 bytes from the arena's
base, so that no operand is aligned to more than the 32 bytes of one value.  upload() sends the image in one copy; check()
downloads the whole arena in one copy and asserts that the listed outputs hold the expected values and that every other byte is
the one that was uploaded: inputs, guards, stride gaps and the unused tail of an output region.

The engine is passed in.  What is used of it: dev_alloc(nbytes) -> address, dev_free(address), dev_upload(address, array) and
engine._lib.kzg_dev_download(engine._h, host address, device address, nbytes) -> 0, so an object backed by a numpy array can
stand in for a context (tests/test_device_arena.py)."""
import ctypes as C

import numpy as np

ROW = 32                 # bytes of one value, the only alignment include/kzg_mi355x.h implies
GUARD_ROWS = 2049        # one more than the largest tile (2048: NTT, combine, linearise, the quotient scan)
GUARD = GUARD_ROWS * ROW  # 64 KiB + 32 B


class Region:
    """rows x cols units of row_bytes each, column j at byte offset + j * stride * row_bytes of the arena"""

    def __init__(self, arena, name, offset, rows, cols, stride, row_bytes):
        self.arena, self.name, self.offset = arena, name, offset
        self.rows, self.cols, self.stride, self.row_bytes = rows, cols, stride, row_bytes

    @property
    def nbytes(self):  # from the first byte of column 0 to the last byte of the last column
        return ((self.cols - 1) * self.stride + self.rows) * self.row_bytes

    @property
    def ptr(self):
        assert self.arena.base is not None, "upload() first: the arena is allocated there"
        return self.arena.base + self.offset

    def col_ptr(self, j):
        return self.ptr + j * self.stride * self.row_bytes

    def _cells(self, image):
        """the (cols, rows * row_bytes) view of this region's own bytes in an arena-sized byte array"""
        return np.lib.stride_tricks.as_strided(image[self.offset:], shape=(self.cols, self.rows * self.row_bytes),
                                               strides=(self.stride * self.row_bytes, 1))

    def _as_bytes(self, values):
        """values for the first rows of every column -> a (cols, r * row_bytes) byte array, r <= rows"""
        a = np.ascontiguousarray(values)
        b = a.view(np.uint8).reshape(self.cols, -1)
        assert b.shape[1] % self.row_bytes == 0 and b.shape[1] <= self.rows * self.row_bytes, (self.name, a.shape)
        return b


class Arena:
    def __init__(self, engine, seed=0):
        self.engine, self.seed = engine, seed
        self.regions, self.base, self.image, self._end, self._inputs = [], None, None, 0, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self.base is not None:
            self.engine.dev_free(self.base)
            self.base = None

    # -- layout --------------------------------------------------------------------------------------------------------------
    def region(self, rows, cols=1, stride=None, name=None, data=None, row_bytes=ROW):
        """Reserves rows x cols (column j starts stride rows after column j - 1; stride None: packed).  data: the input's values,
        (cols, rows, ...) or (rows, ...) for one column; None: an output, which keeps the fill"""
        assert self.base is None, "the layout is fixed by upload()"
        stride = rows if stride is None else stride
        assert rows >= 1 and cols >= 1 and stride >= rows
        offset = self._end + GUARD
        offset += -offset % ROW
        if (offset // ROW) % 2 == 0:
            offset += ROW  # an odd multiple of 32 bytes: aligned to 32 and to nothing more
        r = Region(self, name or "region%d" % len(self.regions), offset, rows, cols, stride, row_bytes)
        self.regions.append(r)
        self._end = offset + r.nbytes
        if data is not None:
            b = r._as_bytes(data)
            assert b.shape[1] == rows * row_bytes, (r.name, "an input fills its region")
            self._inputs.append((r, b.copy()))
        return r

    @property
    def nbytes(self):
        return self._end + (-self._end % ROW) + GUARD

    def upload(self):
        """Builds the image (fill, then the inputs), allocates the arena and sends the image in one copy"""
        assert self.base is None
        self.image = np.random.default_rng(self.seed).integers(0, 256, size=self.nbytes, dtype=np.uint8)
        for r, b in self._inputs:
            r._cells(self.image)[:] = b
        self.image.setflags(write=False)
        self.base = self.engine.dev_alloc(self.nbytes)
        self.engine.dev_upload(self.base, self.image)
        return self

    # -- checks --------------------------------------------------------------------------------------------------------------
    def download(self):
        got = np.zeros(self.nbytes, dtype=np.uint8)
        rc = self.engine._lib.kzg_dev_download(self.engine._h, got.ctypes.data, C.c_void_p(self.base), self.nbytes)
        assert rc == 0, rc
        return got

    def where(self, at):
        """Names the place of byte offset `at`: (text, row, the region if the byte is one of its own values)"""
        for r in self.regions:
            if r.offset <= at < r.offset + r.nbytes:
                col, rel = divmod(at - r.offset, r.stride * r.row_bytes)
                row = rel // r.row_bytes
                column = ", column %d" % col if r.cols > 1 else ""
                if row < r.rows:
                    return "region %s%s" % (r.name, column), row, r
                return "gap of %s, column %d" % (r.name, col), row, None
        best = None  # a guard byte belongs to the nearer region; between two, a tie goes to the one before
        for r in self.regions:
            end = r.offset + r.nbytes
            if at >= end:
                cand = (at - end, 0, "guard after %s" % r.name, (at - end) // ROW)  # row 0: the first row past the end
            else:
                cand = (r.offset - at, 1, "guard before %s" % r.name, (r.offset - at + ROW - 1) // ROW)  # row 1: the last row before
            if best is None or cand[:2] < best[:2]:
                best = cand
        return best[2], best[3], None

    def check(self, outputs=None, unasserted=()):
        """outputs {region: expected values of its first rows, per column}.  unasserted: output regions whose contents are left
        open (error returns); their gaps are still compared.  Returns the downloaded bytes"""
        assert self.base is not None
        got = self.download()
        want = self.image.copy()
        for r, values in (outputs or {}).items():
            b = r._as_bytes(values)
            r._cells(want)[:, :b.shape[1]] = b
        for r in unasserted:
            r._cells(want)[:] = r._cells(got)
        diff = np.flatnonzero(got != want)
        if diff.size:
            places = []
            some = diff if diff.size <= 4096 else np.unique(np.concatenate([diff[:1024], diff[::diff.size // 2048]]))
            for at in some:  # in address order; a sample of them where a whole region is wrong
                place = self.where(int(at))
                if not places or place[0] != places[-1][0]:
                    if len(places) == 6:
                        break
                    places.append(place)
            text, row, inside = places[0]
            kind = "differs from the expected output" if inside in (outputs or {}) else "was written"
            raise AssertionError("%s, row %d %s (byte %d of the arena); %d bytes differ in all, first in: %s" % (
                text, row, kind, int(diff[0]), diff.size, "; ".join("%s row %d" % p[:2] for p in places)))
        return got

    def check_untouched(self):
        """for calls that only read caller memory, and for error returns with no output region"""
        return self.check()
