"""SRS ingest, read-back and the file cache at their boundaries.

Every form in which an SRS reaches the device -- kzg_srs_load_g1 (Jacobian rows at a stride), kzg_srs_load_affine,
kzg_srs_load_compressed, kzg_srs_save -> kzg_srs_load_file -- at the sizes where the ingest kernels change path (32 points
per lane and 2048 per workgroup of k_normalize, 64 per workgroup of k_uncompress, 256 of k_affine96_to_table, 65536 per
chunk of kzg_srs_save), with the point at infinity at the edges of a lane's 32 points; the window tables level by level;
the least bad index of the compressed form on one device and over the slices of a multi-device context; corrupted cache
files whose fingerprints are intact; and the raw little-endian door of the MSM.

Expected values never come from the library: points are the C oracle's SRS (oracle.srs_g1 / srs_g1_at), their bytes
oracle.p1_compress, multiples oracle.p1_mult; the inputs are built by tests/srs_ingest_cases.py, which
tests/test_srs_ingest.py checks against the oracle on the CPU.  Everything is compared bit for bit.
"""
import ctypes as C
import random
import re

import numpy as np
import pytest

import kzg_poly_commit_exploration_amd as K
import srs_ingest_cases as SC
import trapdoor_oracle as TO
import wire_oracle as W

pytestmark = pytest.mark.gpu

R = K.R_MODULUS
SECRET = SC.SECRET_BE
SECRET_INT = int.from_bytes(SECRET, "big") % R
OTHER_SECRET = (0x5EED5EED5EED).to_bytes(32, "big")  # what an engine holds before each load under test
FORMS = ("jacobian/144", "jacobian/432", "affine", "compressed", "file")


# ---------------------------------------------------------------- fixtures and helpers

@pytest.fixture(scope="module")
def srs(oracle):
    return SC.oracle_srs(oracle, max(SC.NS))


@pytest.fixture(scope="module")
def eng():
    e = K.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_b():
    e = K.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def multi():
    """the two kinds of multi-device context, as virtual slices of device 0"""
    m = {"range3": K.Engine(devices=[0, 0, 0]), "replicate2": K.Engine(devices=[0, 0], replicate=True)}
    yield m
    for e in m.values():
        e.close()


def last_error(e):
    return e._lib.kzg_last_error(e._h).decode()


def names_index(message, index):
    return re.search(r"\bpoint %d\b" % index, message) is not None


def refused(fn, status):
    with pytest.raises(K.KzgError) as ei:
        fn()
    assert ei.value.status == status, (ei.value.status, str(ei.value))
    return ei.value


def read_rc(e, index, count):
    """kzg_srs_read_g1's own answer (the wrapper raises): (status, rows)"""
    out = np.zeros((max(count, 1), 18), dtype=np.uint64)
    rc = e._lib.kzg_srs_read_g1(e._h, index, count, out.ctypes.data_as(C.c_void_p))
    return rc, out[:count]


def scramble(e, n):
    """another SRS of the same length, generated on the device: a load that leaves records unwritten shows them"""
    e.srs_generate(OTHER_SECRET, n)


def first_diff(got, want):
    rows = np.nonzero((np.asarray(got) != np.asarray(want)).any(axis=1))[0]
    return int(rows[0]) if rows.size else None


def check_read(oracle, got, case, what, compress=True):
    """the properties of a read-back: the expected words (x, y canonical, Z = Montgomery one, infinity all zero) and, for
    the first form of a case, the oracle's compressed bytes point by point"""
    want = case.expected_read()
    assert got.shape == want.shape, what
    d = first_diff(got, want)
    assert d is None, "%s: srs_read differs first at index %d (infinity there: %s)" % (what, d, d in case.inf)
    finite = np.array([i not in case.inf for i in range(case.n)], dtype=bool)
    assert (got[finite, 12:] == SC.ONE_ROW).all(), what + ": Z of a finite point is not the Montgomery one"
    assert not got[~finite].any(), what + ": an infinity is not all zero"
    if compress:
        encs = case.compressed()
        for i in range(case.n):
            assert oracle.p1_compress(got[i]) == encs[i], "%s: point %d is not the oracle's" % (what, i)


def random_values(rnd, n):
    return [rnd.randrange(R) for _ in range(n)]


def want_commit(oracle, vals, inf=()):
    """[sum_{i not infinity} v_i s^i] G: the commitment over the oracle's SRS for SECRET with infinities at `inf`"""
    kept = [0 if i in inf else v for i, v in enumerate(vals)]
    return TO.g1_scalar(oracle, TO.poly_eval(kept, SECRET_INT))


def check_commit(oracle, e, case, rnd, what):
    vals = random_values(rnd, case.n)
    got = e.commit_limbs(K.scalars_to_limbs(vals)).compress()
    assert got == want_commit(oracle, vals, case.inf), what + ": commitment differs from the oracle's"


def load_form(form, e, helper, case, tmp_path, what):
    """brings `case` into engine e through one form; `helper` is the engine the file form saves from"""
    if form == "jacobian/144":
        rows = case.jacobian(144, seed=case.n)
        assert rows.strides[0] == 144
        e.srs_load(rows)
    elif form == "jacobian/432":
        rows = case.jacobian(432, seed=case.n + 1)  # the other infinity variant at every position
        assert rows.strides[0] == 432
        e.srs_load(rows)
    elif form == "affine":
        e.srs_load_affine(case.affine())
    elif form == "compressed":
        e.srs_load_compressed(case.compressed_blob())
    elif form == "file":
        path = str(tmp_path / "srs.bin")
        helper.srs_load_affine(case.affine())
        helper.srs_save(path)
        with open(path, "rb") as fh:
            data = fh.read()
        want = SC.srs_file_bytes(case.affine())
        assert len(data) == len(want), what
        assert data[:128] == want[:128], what + ": header of the saved file"
        assert data == want, what + ": body of the saved file"
        if helper is e:  # saved from the engine under test: it must not pass by still holding what it saved
            scramble(e, case.n)
        e.srs_load_file(path)
    else:
        raise KeyError(form)


# ---------------------------------------------------------------- 1. every form, every size, every infinity pattern

@pytest.mark.parametrize("n", SC.NS)
def test_every_form_reads_back_the_oracle_points(oracle, srs, eng, eng_b, tmp_path, n):
    for pattern in SC.patterns_for(n):
        case = SC.Case(oracle, srs[:n], SC.infinity_set(pattern, n))
        reads = {}
        for form in FORMS:
            what = "form %s, n = %d, pattern %s" % (form, n, pattern)
            scramble(eng, n)
            load_form(form, eng, eng_b, case, tmp_path, what)
            assert eng.srs_len() == n, what
            got = eng.srs_read(0, n)
            check_read(oracle, got, case, what, compress=not reads)
            reads[form] = got
        base = reads[FORMS[0]]
        for form in FORMS[1:]:  # the read-back is canonical: equal points are equal words
            d = first_diff(reads[form], base)
            assert d is None, "forms %s and %s, n = %d, pattern %s: read-backs differ first at index %d" % (
                FORMS[0], form, n, pattern, d)


# ---------------------------------------------------------------- 2. table levels, point by point

def single_digit_at(v, c, levels, j):
    """does v recode (msm_sort.hip: fold, then signed c-bit windows) to the one digit +1 at level j?"""
    if v >= R or c * j >= 254:
        return False
    mag, negated = TO.fold(v)
    if negated:
        return False
    digits = TO.window_digits(mag, c, levels)
    return digits[j] == 1 and not any(d for t, d in enumerate(digits) if t != j)


@pytest.mark.parametrize("n", [33, 2049])
def test_table_levels_point_by_point(oracle, srs, eng, n):
    """level j of point i is [2^(c j)] SRS[i]: a loaded infinity stays infinity on every level, its neighbours are
    untouched on every level"""
    inf = frozenset({31, 32, n - 1})
    case = SC.Case(oracle, srs[:n], inf)
    scramble(eng, n)
    eng.srs_load(case.jacobian(144, seed=3))
    cfg = eng.msm_config()
    c, levels = cfg["digit_bits"], cfg["table_levels"]
    assert cfg["recoding"] == "windows" and levels == TO.windows_of(c)
    usable = [j for j in range(levels) if single_digit_at(1 << (c * j), c, levels, j)]
    assert usable[:levels - 1] == list(range(levels - 1)), "only the top level may be out of a single digit's reach"
    indices = sorted({i for i in (0, 30, 31, 32, 33, n - 2, n - 1) if 0 <= i < n})
    assert inf <= set(indices)
    for i in indices:
        for j in usable:
            v = 1 << (c * j)
            coeffs = np.zeros((n, 4), dtype=np.uint64)
            coeffs[i] = K.scalars_to_limbs([v])[0]
            got = eng.commit_limbs(coeffs).compress()
            want = SC.INF_48 if i in inf else oracle.p1_compress(oracle.p1_mult(srs[i], v))
            assert got == want, "n = %d, point %d, level %d (c = %d)" % (n, i, j, c)
    # one dense commitment: the infinities contribute nothing
    vals = random_values(random.Random(n), n)
    kept = [0 if i in inf else v for i, v in enumerate(vals)]
    rc, want = oracle.commit_naive(K.scalars_to_limbs(kept), srs[:n])
    assert rc == 0
    assert eng.commit_limbs(K.scalars_to_limbs(vals)).compress() == oracle.p1_compress(want), n


# ---------------------------------------------------------------- 3. least bad index of the compressed form

def bad_encodings():
    """(class, 48 bytes) of every malformed encoding of wire_oracle; an abscissa off the curve only when the host's
    uncompress refuses it as well"""
    out = []
    for name, enc in W.malformed_points().items():
        if name == "not on the curve":
            try:
                K.G1Point.uncompress(enc)
                continue
            except K.KzgError:
                pass
        out.append((name, enc))
    return out


# (n, bad positions, infinity positions)
BAD_CASES = [
    (1, (0,), ()),
    (65, (0,), ()),
    (65, (63,), ()),
    (65, (64,), ()),          # the second workgroup of k_uncompress, and the last point
    (2049, (0,), ()),
    (2049, (63,), ()),
    (2049, (64,), ()),
    (2049, (2048,), ()),
    (2049, (64, 1500), ()),   # two workgroups: the lesser
    (2049, (2048, 1), ()),
    (2049, (64,), (10, 63)),  # an infinity is not malformed
]


def plant(blob, positions, encodings):
    out = bytearray(blob)
    for k, (at, enc) in enumerate(zip(positions, encodings)):
        out[48 * at:48 * at + 48] = enc
    return bytes(out)


def assert_holds_no_srs(e, n, what, opening=True):
    assert e.srs_len() == 0, what
    coeffs = K.scalars_to_limbs([1] * n)
    refused(lambda: e.commit_limbs(coeffs), K.KZG_ERR_NO_SRS)
    rc, _ = read_rc(e, 0, 1)
    assert rc == K.KZG_ERR_NO_SRS, (what, rc)
    rc, _ = read_rc(e, 0, 0)
    assert rc == K.KZG_ERR_NO_SRS, (what, rc)
    if opening:
        refused(lambda: e.open_limbs(K.scalars_to_limbs([1, 1]), K.Scalar(0), K.Scalar(1)), K.KZG_ERR_NO_SRS)
    refused(e.msm_config, K.KZG_ERR_NO_SRS)


def test_compressed_load_reports_the_least_bad_index(oracle, srs, eng):
    kinds = bad_encodings()
    assert len(kinds) >= 5
    rnd = random.Random(33)
    turn = 0
    for n, bad, inf in BAD_CASES:
        case = SC.Case(oracle, srs[:n], inf)
        encs = []
        for _ in bad:
            encs.append(kinds[turn % len(kinds)])
            turn += 1
        what = "n = %d, bad %s (%s), infinity %s" % (n, bad, ", ".join(k for k, _ in encs), inf)
        scramble(eng, n)
        blob = plant(case.compressed_blob(), bad, [e for _, e in encs])
        err = refused(lambda: eng.srs_load_compressed(blob), K.KZG_ERR_INVALID_ARG)
        assert err.bad_index == min(bad), what
        assert names_index(last_error(eng), min(bad)), (what, last_error(eng))
        assert_holds_no_srs(eng, n, what)
    # a good load on the same engine afterwards
    case = SC.Case(oracle, srs[:2049], (10, 63))
    eng.srs_load_compressed(case.compressed_blob())
    check_read(oracle, eng.srs_read(0, case.n), case, "good load after the refusals", compress=False)
    check_commit(oracle, eng, case, rnd, "good load after the refusals")


# ---------------------------------------------------------------- 4. multi-device contexts

def slice_starts(n, k=3):
    """multi.hip shard_range: the first point of every slice but the first"""
    per = (n + k - 1) // k
    return [g * per for g in range(1, k) if g * per < n]


def boundary_infinities(n):
    """an infinity on each side of every slice boundary of the three-way split"""
    return frozenset(i for b in slice_starts(n) for i in (b - 1, b))


@pytest.mark.parametrize("n", [1, 2, 3, 100, 2049])
@pytest.mark.parametrize("kind", ["range3", "replicate2"])
def test_multi_device_context_every_form(oracle, srs, multi, eng_b, tmp_path, kind, n):
    m = multi[kind]
    rnd = random.Random(n)
    infs = [boundary_infinities(n)]
    if n <= 3:  # there the boundaries leave no finite point (n = 2, 3) or no infinity (n = 1): also the other extreme
        infs.append(frozenset() if infs[0] else frozenset({0}))
    for inf in infs:
        case = SC.Case(oracle, srs[:n], inf)
        reads = []
        for form in FORMS:
            what = "%s, form %s, n = %d, infinity %s" % (kind, form, n, sorted(inf))
            scramble(m, n)
            load_form(form, m, m if form == "file" and kind == "range3" else eng_b, case, tmp_path, what)
            assert m.srs_len() == n, what
            rc, got = read_rc(m, 0, n)  # one read over all the slices
            assert rc == K.KZG_OK, what
            check_read(oracle, got, case, what, compress=not reads)
            reads.append(got)
            assert read_rc(m, n, 0)[0] == K.KZG_OK, what + ": an empty read at the end"
            assert read_rc(m, n, 1)[0] == K.KZG_ERR_INVALID_ARG, what
            assert read_rc(m, 0, n + 1)[0] == K.KZG_ERR_INVALID_ARG, what
            assert read_rc(m, n + 1, 0)[0] == K.KZG_ERR_INVALID_ARG, what
            for b in slice_starts(n):  # a read that starts or ends on a boundary, and one across it
                lo, hi = max(b - 2, 0), min(b + 2, n)
                for i0, i1 in ((lo, b), (b, hi), (lo, hi)):
                    rc, part = read_rc(m, i0, i1 - i0)
                    assert rc == K.KZG_OK and np.array_equal(part, got[i0:i1]), (what, i0, i1)
            check_commit(oracle, m, case, rnd, what)


@pytest.mark.parametrize("kind", ["range3", "replicate2"])
def test_multi_device_context_reports_the_global_bad_index(oracle, srs, multi, kind):
    """n = 100 splits into [0, 34), [34, 68), [68, 100): a bad point in slice 1 only, in slice 2 only, in both; at 2049 the
    slices are 683 long, more than a workgroup of k_uncompress each"""
    m = multi[kind]
    kinds = bad_encodings()
    rnd = random.Random(5)
    turn = 0
    for n, bad in ((100, (40,)), (100, (99,)), (100, (68,)), (100, (80, 67)), (100, (34, 68)),
                   (2049, (683,)), (2049, (2048,)), (2049, (1366 + 70, 683 + 65))):
        starts = slice_starts(n)
        assert all(b >= starts[0] for b in bad), "nothing malformed in slice 0"
        case = SC.Case(oracle, srs[:n], ())
        encs = []
        for _ in bad:
            encs.append(kinds[turn % len(kinds)])
            turn += 1
        what = "%s, n = %d, bad %s (%s)" % (kind, n, bad, ", ".join(k for k, _ in encs))
        scramble(m, n)
        blob = plant(case.compressed_blob(), bad, [e for _, e in encs])
        err = refused(lambda: m.srs_load_compressed(blob), K.KZG_ERR_INVALID_ARG)
        assert err.bad_index == min(bad), what
        assert names_index(last_error(m), min(bad)), (what, last_error(m))
        assert_holds_no_srs(m, n, what)
    case = SC.Case(oracle, srs[:100], boundary_infinities(100))
    m.srs_load_compressed(case.compressed_blob())
    check_read(oracle, m.srs_read(0, 100), case, kind + ": good load after the refusals", compress=False)
    check_commit(oracle, m, case, rnd, kind + ": good load after the refusals")


def test_multi_device_context_saves_the_same_file(oracle, srs, multi, eng, tmp_path):
    """kzg_srs_save stitches the slices: byte for byte the single-device engine's file"""
    for n in (2, 100, 2049):
        case = SC.Case(oracle, srs[:n], boundary_infinities(n))
        rows = case.jacobian(144, seed=n)
        files = []
        for name, e in (("single", eng), ("range3", multi["range3"])):
            scramble(e, n)
            e.srs_load(rows)
            path = str(tmp_path / ("%s_%d.bin" % (name, n)))
            e.srs_save(path)
            with open(path, "rb") as fh:
                files.append(fh.read())
        assert files[0] == files[1], n
        assert files[0] == SC.srs_file_bytes(case.affine()), n


# ---------------------------------------------------------------- 5. the file cache

def oracle_affine(oracle, row):
    out = oracle.p1_zeros(1)
    src = np.ascontiguousarray(row, dtype=np.uint64)
    oracle.lib().oracle_p1_to_affine(out.ctypes.data, src.ctypes.data)
    return out[0, :12]


def test_save_in_two_chunks(oracle, eng, eng_b, tmp_path):
    """n = 65537: kzg_srs_save writes 65536 points and then one; the header's `last` comes from the second chunk"""
    n = SC.SAVE_CHUNK + 1
    eng.srs_generate(SECRET, n)
    path = str(tmp_path / "two_chunks.bin")
    eng.srs_save(path)
    with open(path, "rb") as fh:
        data = fh.read()
    assert len(data) == 128 + 96 * n
    f = SC.parse_srs_file(data)
    assert f["magic"] == SC.MAGIC and f["n"] == n and f["reserved"] == bytes(16)
    assert f["first"] == oracle.p1_compress(oracle.srs_g1_at(0, SECRET)), "first fingerprint"
    assert f["last"] == oracle.p1_compress(oracle.srs_g1_at(n - 1, SECRET)), "last fingerprint"
    rnd = random.Random(65537)
    for i in [0, SC.SAVE_CHUNK - 1, SC.SAVE_CHUNK] + [rnd.randrange(n) for _ in range(64)]:
        assert np.array_equal(f["rows"][i], oracle_affine(oracle, oracle.srs_g1_at(i, SECRET))), i
    scramble(eng_b, 33)
    eng_b.srs_load_file(path)
    assert eng_b.srs_len() == n
    back = eng_b.srs_read(0, n)
    d = first_diff(back, eng.srs_read(0, n))
    assert d is None, "read-back of the loaded file differs first at index %d" % d
    assert np.array_equal(back[:, :12], f["rows"])


def test_file_round_trip_with_infinity_at_the_ends(oracle, srs, eng, eng_b, tmp_path):
    n = 33
    # secret 0: [G, infinity, infinity, ...] -- the last fingerprint is infinity
    eng.srs_generate(bytes(32), n)
    case = SC.Case(oracle, srs[:n], range(1, n))
    check_read(oracle, eng.srs_read(0, n), case, "generated with secret 0")
    path = str(tmp_path / "zero_secret.bin")
    eng.srs_save(path)
    with open(path, "rb") as fh:
        data = fh.read()
    assert data == SC.srs_file_bytes(case.affine())
    f = SC.parse_srs_file(data)
    assert f["last"] == SC.INF_48 and f["first"] == oracle.p1_compress(oracle.p1_generator())
    scramble(eng_b, n)
    eng_b.srs_load_file(path)
    check_read(oracle, eng_b.srs_read(0, n), case, "secret 0 through the file", compress=False)
    # a loaded SRS whose first point is infinity
    case = SC.Case(oracle, srs[:n], {0})
    eng.srs_load(case.jacobian(144, seed=1))
    path = str(tmp_path / "first_infinity.bin")
    eng.srs_save(path)
    with open(path, "rb") as fh:
        data = fh.read()
    assert data == SC.srs_file_bytes(case.affine())
    assert SC.parse_srs_file(data)["first"] == SC.INF_48
    scramble(eng_b, n)
    eng_b.srs_load_file(path)
    check_read(oracle, eng_b.srs_read(0, n), case, "infinity first, through the file", compress=False)
    check_commit(oracle, eng_b, case, random.Random(1), "infinity first, through the file")


def resident_case(oracle, srs, e):
    """an SRS the engine holds while files are refused"""
    case = SC.Case(oracle, srs[:65], {64})
    e.srs_load_affine(case.affine())
    return case


def assert_still_resident(oracle, e, case, rnd, what):
    assert e.srs_len() == case.n, what
    check_read(oracle, e.srs_read(0, case.n), case, what + ": the previous SRS", compress=False)
    check_commit(oracle, e, case, rnd, what + ": the previous SRS")


def off_curve(row):
    """y + 1"""
    out = row.copy()
    out[6:] = SC.fp_row(SC.T.fp_from_mont_limbs([int(v) for v in row[6:]]) + 1)
    return out


def plus_p(row, which):
    """x (which = 0) or y (which = 1) replaced by itself + p: the same residue, no longer below p, still 384 bits"""
    out = row.copy()
    out[6 * which:6 * which + 6] = SC.raw_row(SC.row_int(row[6 * which:6 * which + 6]) + SC.P)
    return out


def test_corrupted_file_with_intact_fingerprints_is_refused(oracle, srs, eng, tmp_path):
    rnd = random.Random(77)
    held = resident_case(oracle, srs, eng)
    small = SC.Case(oracle, srs[:257], {5}).affine()
    # 65537 points without 65537 scalar multiplications: the 4097 oracle points over and over (a cache file need not hold
    # powers of one secret); kzg_srs_load_file spreads its on-curve check over up to 16 threads, thread t taking i = t mod 16
    big = np.tile(SC.Case(oracle, srs, ()).affine(), (17, 1))[:SC.SAVE_CHUNK + 1]
    files = []

    def corrupt(rows, changes, name):
        rows = rows.copy()
        for at, fn in changes:
            assert 0 < at < rows.shape[0] - 1, "the fingerprints stay intact"
            rows[at] = fn(rows[at])
        files.append((name, min(at for at, _ in changes), SC.srs_file_bytes(rows)))

    corrupt(small, [(128, off_curve)], "y + 1 in the middle")
    corrupt(small, [(200, lambda r: plus_p(r, 0))], "x + p")
    corrupt(small, [(6, lambda r: plus_p(r, 1))], "y + p, next to an infinity")
    # the greater index has the lesser residue mod 16: the thread that meets it comes first in thread order
    corrupt(big, [(50002, off_curve), (20005, lambda r: plus_p(r, 0))], "two points, residues 2 and 5 mod 16")
    corrupt(big, [(SC.SAVE_CHUNK - 1, off_curve)], "the last point of the first chunk")
    path = str(tmp_path / "corrupt.bin")
    for name, least, data in files:
        with open(path, "wb") as fh:
            fh.write(data)
        refused(lambda: eng.srs_load_file(path), K.KZG_ERR_INVALID_ARG)
        assert names_index(last_error(eng), least), (name, least, last_error(eng))
        assert_still_resident(oracle, eng, held, rnd, name)
    # the same files without the corruption load
    for rows in (small, big):
        with open(path, "wb") as fh:
            fh.write(SC.srs_file_bytes(rows))
        eng.srs_load_file(path)
        assert eng.srs_len() == rows.shape[0]
        assert np.array_equal(eng.srs_read(0, rows.shape[0])[:, :12], rows)


def test_file_header_errors_are_refused(oracle, srs, eng, tmp_path):
    rnd = random.Random(78)
    held = resident_case(oracle, srs, eng)
    n = 100
    rows = SC.Case(oracle, srs[:n], ()).affine()
    enc = SC.affine_row_compress
    good = SC.srs_file_bytes(rows)
    files = {
        "header n larger than the file": SC.srs_file_bytes(rows, header_n=n + 1),
        # ... with the fingerprint of the point the header calls the last, so that only the length can refuse it
        "header n smaller than the file": SC.srs_file_bytes(rows, header_n=n - 1, last=enc(rows[n - 2])),
        "n = 0, no body": SC.srs_file_bytes(rows, header_n=0)[:128],
        "n = 0, with a body": SC.srs_file_bytes(rows, header_n=0),
        "wrong last fingerprint": SC.srs_file_bytes(rows, last=enc(rows[n - 2])),
        "wrong first fingerprint": SC.srs_file_bytes(rows, first=enc(rows[1])),
        "last fingerprint infinity": SC.srs_file_bytes(rows, last=SC.INF_48),
    }
    path = str(tmp_path / "header.bin")
    for name, data in files.items():
        assert data != good
        with open(path, "wb") as fh:
            fh.write(data)
        refused(lambda: eng.srs_load_file(path), K.KZG_ERR_INVALID_ARG)
        assert_still_resident(oracle, eng, held, rnd, name)
    with open(path, "wb") as fh:
        fh.write(good)
    eng.srs_load_file(path)
    assert np.array_equal(eng.srs_read(0, n)[:, :12], rows)


# ---------------------------------------------------------------- 6. raw little-endian scalars

def le_bytes(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def edge_scalars():
    half = TO.HALF
    band = R >> 31
    near = [half - band, half - band + 1, half - 1, half + 2, half + band, half + 1 + band, half + 1 + band - 1, half - 5]
    assert all(TO.near_fold_boundary(v) for v in near)
    assert not TO.near_fold_boundary(half - band - 1) and not TO.near_fold_boundary(half + 2 + band)
    return [0, 1, R - 1, (R - 1) // 2, (R + 1) // 2] + near


# msm_sort.hip launch_bucket_sort: one polynomial of at most kSmallSortScalars = 4096 scalars on a table of at most
# kSmallSortBuckets = 4096 buckets is sorted by k_sort_small; anything longer takes the general path
# (k_sort_count, k_sort_spread ...).  n = 1025 takes the first (its SRS has 2^7 buckets), n = 4097 the second.
@pytest.mark.parametrize("n,small_sort", [(1025, True), (4097, False)])
def test_commit_le_bytes_at_the_recoding_edges_and_above_r(oracle, eng, n, small_sort):
    eng.srs_generate(SECRET, n)
    buckets = eng.msm_config()["buckets"]
    assert (n <= 4096 and buckets <= 4096) == small_sort, (n, buckets)
    rnd = random.Random(n)
    vals = random_values(rnd, n)
    edges = edge_scalars()
    places = rnd.sample(range(n), 4 * len(edges))
    for k, at in enumerate(places):
        vals[at] = edges[k % len(edges)]
    vals[0], vals[n - 1] = (R - 1) // 2, (R + 1) // 2
    want = TO.commitment(oracle, vals, SECRET_INT)
    assert eng.commit_le_bytes(le_bytes(vals)).compress() == want, "canonical raw scalars"
    assert eng.commit_limbs(K.scalars_to_limbs(vals)).compress() == want, "the same values as blst_fr"
    # the same polynomial with entries at or above r: every one of its values again plus r (r < 2^255, so it fits), plus
    # 2 r where that fits, and 2^256 - 1
    top = (1 << 256) - 1
    raw = list(vals)
    for at in range(n):
        turn = at % 4
        if turn == 0:
            raw[at] = vals[at] + R
        elif turn == 1 and vals[at] + 2 * R <= top:
            raw[at] = vals[at] + 2 * R
    for at in places[:8]:
        raw[at] = top
    raw[1] = R  # zero
    raw[2] = top
    assert all(0 <= v <= top for v in raw) and sum(v >= R for v in raw) > n // 4
    reduced = [v % R for v in raw]
    want = TO.commitment(oracle, reduced, SECRET_INT)
    assert eng.commit_limbs(K.scalars_to_limbs(reduced)).compress() == want
    assert eng.commit_le_bytes(le_bytes(reduced)).compress() == want, "reduced by the caller"
    assert eng.commit_le_bytes(le_bytes(raw)).compress() == want, "raw scalars at or above r commit to the values mod r"
