"""CPU: tests/device_arena.py against an engine that is a numpy array.  A "call" that writes exactly its output passes; each
planted stray store fails and is reported at the right region and row.  This is what shows that the cases of
tests/test_device_bounds_gpu.py would fail if a kernel wrote outside its output."""
import ctypes as C
import re

import numpy as np
import pytest

import device_arena as DA

N, COLS, STRIDE = 37, 3, 37 + 5


class FakeEngine:
    """dev_alloc hands out the address of a numpy byte array; the "kernels" of these tests store through mem(address)"""

    def __init__(self):
        self._lib, self._h, self.bufs = self, None, {}

    def dev_alloc(self, nbytes):
        buf = np.zeros(nbytes, dtype=np.uint8)
        self.bufs[buf.ctypes.data] = buf
        return buf.ctypes.data

    def dev_free(self, dptr):
        del self.bufs[dptr]

    def mem(self, dptr, nbytes):
        for base, buf in self.bufs.items():
            if base <= dptr and dptr + nbytes <= base + buf.size:
                return buf[dptr - base:dptr - base + nbytes]
        raise AssertionError("address outside every allocation")

    def dev_upload(self, dptr, array):
        a = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
        self.mem(dptr, a.size)[:] = a

    def kzg_dev_download(self, h, dst, src, nbytes):
        C.memmove(dst, self.mem(src.value, nbytes).ctypes.data, nbytes)
        return 0


def _values(rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 2**63, size=(cols, rows, 4), dtype=np.uint64)


class Case:
    """inp (strided) | out (strided) | tail (one column), the output between the two inputs"""

    def __init__(self):
        self.eng = FakeEngine()
        self.arena = DA.Arena(self.eng, seed=5)
        self.a, self.want = _values(N, COLS, 1), _values(N, COLS, 2)
        self.inp = self.arena.region(N, COLS, STRIDE, name="inp", data=self.a)
        self.out = self.arena.region(N, COLS, STRIDE, name="out")
        self.tail = self.arena.region(N, name="tail", data=self.a[0])
        self.arena.upload()

    def store(self, ptr, rows):
        """what a kernel does: rows of 32 bytes at a device address"""
        b = np.ascontiguousarray(rows).view(np.uint8).reshape(-1)
        self.eng.mem(ptr, b.size)[:] = b

    def call(self, stride=STRIDE):
        for j in range(COLS):
            self.store(self.out.ptr + j * stride * 32, self.want[j])

    def fails(self, place, row, nbytes=None, **kw):
        with pytest.raises(AssertionError) as ei:
            self.arena.check(**(kw or {"outputs": {self.out: self.want}}))
        text = str(ei.value)
        assert text.startswith("%s, row %d " % (place, row)), text
        if nbytes is not None:
            assert int(re.search(r"(\d+) bytes differ", text).group(1)) == nbytes, text
        return text


@pytest.fixture
def case():
    c = Case()
    yield c
    c.arena.close()
    assert not c.eng.bufs  # close() frees the one allocation


def test_layout_guards_alignment_and_fill(case):
    ar = case.arena
    assert DA.GUARD_ROWS == 2049 and DA.GUARD == 64 * 1024 + 32
    end = 0
    for r in ar.regions:
        assert r.offset - end >= DA.GUARD  # a whole band before every region
        assert r.offset % 32 == 0 and (r.offset // 32) % 2 == 1  # an odd multiple of 32 bytes: never 64-byte aligned
        assert r.ptr == ar.base + r.offset and r.col_ptr(1) == r.ptr + r.stride * 32
        end = r.offset + r.nbytes
    assert ar.nbytes - end >= DA.GUARD and len(case.eng.bufs) == 1
    img = ar.image
    assert np.array_equal(case.inp._cells(img).view(np.uint64).reshape(COLS, N, 4), case.a)  # inputs are in the image
    # the fill is not constant, not zero and not periodic in rows: no shifted copy of it equals it
    guard = img[:DA.GUARD].reshape(-1, 32)
    assert len({bytes(row) for row in guard}) == DA.GUARD_ROWS and guard.any(axis=1).all()
    with DA.Arena(case.eng, seed=6) as other:  # seeded
        other.region(1)
        assert not np.array_equal(other.upload().image[:64], img[:64])


def test_exact_call_passes(case):
    case.call()
    case.arena.check(outputs={case.out: case.want})
    with pytest.raises(AssertionError):  # and the output is compared: a wrong value does not pass
        bad = case.want.copy()
        bad[1, 7, 2] ^= np.uint64(1 << 40)
        case.arena.check(outputs={case.out: bad})


def test_untouched_passes_and_unused_output_tail_is_fill(case):
    case.arena.check_untouched()
    for j in range(COLS):  # a call that writes the first N - 3 rows of each column only
        case.store(case.out.col_ptr(j), case.want[j, :N - 3])
    case.arena.check(outputs={case.out: case.want[:, :N - 3]})
    case.store(case.out.col_ptr(2) + (N - 1) * 32, case.want[2, :1])  # and one that also touches the unused tail
    case.fails("region out, column 2", N - 1, outputs={case.out: case.want[:, :N - 3]})


def test_wrong_output_value_names_region_column_and_row(case):
    case.call()
    case.store(case.out.col_ptr(1) + 9 * 32 + 5, np.array([case.want[1, 9].view(np.uint8)[5] ^ 1], dtype=np.uint8))
    text = case.fails("region out, column 1", 9, nbytes=1)
    assert "differs from the expected output" in text


def test_one_row_past_the_end(case):
    case.call()
    case.store(case.out.ptr + case.out.nbytes, case.want[0, :1])
    case.fails("guard after out", 0)


def test_one_row_before_the_output(case):
    case.call()
    case.store(case.out.ptr - 32, case.want[0, :1])
    case.fails("guard before out", 1)


def test_row_in_a_stride_gap(case):
    case.call()
    case.store(case.out.col_ptr(1) + (N + 2) * 32, case.want[0, :1])
    case.fails("gap of out, column 1", N + 2)


def test_zero_filled_row_in_a_guard(case):
    case.call()
    case.store(case.inp.ptr - 700 * 32, np.zeros(4, dtype=np.uint64))
    case.fails("guard before inp", 700)


def test_one_changed_byte_in_an_input(case):
    case.call()
    cell = case.eng.mem(case.inp.col_ptr(2) + 11 * 32 + 31, 1)
    cell[0] ^= 0x80
    text = case.fails("region inp, column 2", 11, nbytes=1)
    assert "was written" in text
    cell[0] ^= 0x80
    case.arena.check(outputs={case.out: case.want})  # put back: clean again


def test_output_written_at_stride_n_instead_of_the_declared_stride(case):
    case.call(stride=N)
    # column 1 then starts 5 rows early, in the gap after column 0
    case.fails("gap of out, column 0", N)


def test_write_2048_rows_past_the_end_is_inside_the_band(case):
    case.call()
    case.store(case.tail.ptr + case.tail.nbytes + 2048 * 32, case.want[0, :1])
    case.fails("guard after tail", 2048)
    # between two regions the band is attributed to the nearer one
    at = case.tail.offset + case.tail.nbytes + 2048 * 32
    case.store(case.arena.base + at, case.arena.image[at:at + 32])  # put back
    at = case.out.offset + case.out.nbytes + 2048 * 32
    case.store(case.arena.base + at, case.want[0, :1])
    case.fails("guard before tail", (case.tail.offset - at) // 32)


def test_error_returns_leave_the_output_open_but_nothing_else(case):
    case.store(case.out.col_ptr(0), case.want[0, :4])  # a call that gave up part-way
    case.arena.check(unasserted=[case.out])
    case.store(case.out.col_ptr(0) + N * 32, case.want[0, :1])  # the gap is not part of the output
    case.fails("gap of out, column 0", N, unasserted=[case.out])


def test_regions_of_words_end_mid_row():
    eng = FakeEngine()
    with DA.Arena(eng) as ar:
        k, n = 3, 257
        rows = ar.region(n, k, name="rows", row_bytes=4)  # k * n 32-bit words, packed
        after = ar.region(4, name="after", data=_values(4, 1, 3))
        ar.upload()
        assert rows.nbytes == k * n * 4 and rows.nbytes % 32 != 0 and after.offset - (rows.offset + rows.nbytes) >= DA.GUARD
        want = np.arange(k * n, dtype=np.uint32).reshape(k, n)
        eng.dev_upload(rows.ptr, want)
        ar.check(outputs={rows: want})
        eng.mem(rows.ptr + rows.nbytes, 4)[:] = 0  # one word more
        with pytest.raises(AssertionError) as ei:
            ar.check(outputs={rows: want})
        assert str(ei.value).startswith("guard after rows, row 0 "), ei.value
    assert not eng.bufs
