"""The input builders of the SRS ingest tests (tests/srs_ingest_cases.py) against the C oracle, on the CPU: the GPU tests
(tests/test_srs_ingest_gpu.py) compare the library with these inputs, so the inputs are checked first."""
import numpy as np
import pytest

import srs_ingest_cases as SC

N = 97  # three full lanes and one point: every pattern is what its name says


@pytest.fixture(scope="module")
def srs(oracle):
    return SC.oracle_srs(oracle, N)


def test_patterns_cover_the_lane_positions():
    n = 2049
    assert SC.infinity_set("none", n) == frozenset()
    assert SC.infinity_set("first", n) == {0}
    assert SC.infinity_set("lane_end", n) == {31}
    assert SC.infinity_set("lane_start", n) == {32}
    assert SC.infinity_set("last", n) == {n - 1}
    assert SC.infinity_set("whole_lane", n) == set(range(32, 64))
    assert len(SC.infinity_set("all_but_one", n)) == n - 1
    assert SC.infinity_set("all", n) == set(range(n))
    assert SC.infinity_set("whole_lane", 33) == {32} and SC.infinity_set("lane_end", 31) == frozenset()
    for m in SC.NS:
        if m >= 3:  # the survivor is neither the first nor the last point
            (alive,) = set(range(m)) - SC.infinity_set("all_but_one", m)
            assert 0 < alive < m - 1


def test_every_pattern_meets_three_sizes_and_the_two_full_ones():
    sizes = {p: [n for n in SC.NS if p in SC.patterns_for(n)] for p in SC.PATTERNS}
    for p, at in sizes.items():
        assert len(at) >= 3 and 33 in at and 2049 in at, (p, at)
        # ... at sizes where the pattern is not degenerate (an empty set is the pattern "none")
        real = [n for n in at if p == "none" or SC.infinity_set(p, n)]
        assert len(real) >= 3, (p, real)
    for n in SC.NS:
        assert len(SC.patterns_for(n)) >= 2 or n == 1 and SC.patterns_for(n)


@pytest.mark.parametrize("stride", [144, 432])
@pytest.mark.parametrize("pattern", SC.PATTERNS)
def test_jacobian_rows_are_the_oracle_points(oracle, srs, pattern, stride):
    """every rescaled row compresses to the original's bytes; infinity is Z = 0, with junk or without; the factors include
    1, p - 1 and the top-limb-only value"""
    case = SC.Case(oracle, srs, SC.infinity_set(pattern, N), seed=stride)
    rows, kinds = case.jacobian(stride, with_kinds=True)
    assert rows.shape == (N, stride // 8) and rows.strides[0] == stride
    want = case.compressed()
    for i in range(N):
        assert oracle.p1_compress(rows[i, :18]) == want[i], (pattern, i, kinds[i])
        if i in case.inf:
            assert want[i] == SC.INF_48 and not rows[i, 12:18].any()
            assert rows[i, :12].any() == (kinds[i] == "inf_junk")
            if kinds[i] == "inf_junk":
                assert rows[i, :6].any() and rows[i, 6:12].any()
        else:
            assert want[i] == oracle.p1_compress(srs[i]) and rows[i, 12:18].any()
    finite = {k for k in kinds if not isinstance(k, str)}
    if len(case.inf) < N - 4:
        assert finite == {0, 1, 2, 3, 4}
    if len(case.inf) >= 2:
        assert {k for k in kinds if isinstance(k, str)} == {"inf_junk", "inf_zero"}
    if stride > 144:
        assert rows[:, 18:].all(), "the gap of the stride is filled"


def test_rescaling_factors(oracle, srs):
    """a factor of one leaves the row as it is, p - 1 negates Y, and the rows differ from the oracle's where they should"""
    case = SC.Case(oracle, srs, (), seed=0)
    rows, kinds = case.jacobian(144, with_kinds=True)
    for i in range(N):
        same = np.array_equal(rows[i], srs[i])
        assert same == (kinds[i] == 0), (i, kinds[i])
    assert SC.row_int(SC.fp_row(1)) == (1 << 384) % SC.P and SC.row_int(SC.fp_row(SC.P - 1)) == SC.P - (1 << 384) % SC.P
    assert not SC.TOP_LIMB_LAMBDA[:5].any() and SC.TOP_LIMB_LAMBDA[5]


@pytest.mark.parametrize("pattern", SC.PATTERNS)
def test_affine_rows_and_expected_read_are_the_oracle_affine_form(oracle, srs, pattern):
    case = SC.Case(oracle, srs, SC.infinity_set(pattern, N))
    aff, read = case.affine(), case.expected_read()
    lib = oracle.lib()
    for i in range(N):
        if i in case.inf:
            assert not aff[i].any() and not read[i].any()
            continue
        want = oracle.p1_zeros(1)
        src = np.ascontiguousarray(srs[i])
        lib.oracle_p1_to_affine(want.ctypes.data, src.ctypes.data)
        assert np.array_equal(aff[i], want[0, :12]), i
        assert np.array_equal(read[i], want[0]), i  # Z = Montgomery one
        assert lib.oracle_p1_on_curve(np.ascontiguousarray(read[i]).ctypes.data)


@pytest.mark.parametrize("pattern", SC.PATTERNS)
def test_compressed_strings_round_trip(oracle, srs, pattern):
    case = SC.Case(oracle, srs, SC.infinity_set(pattern, N))
    encs = case.compressed()
    assert case.compressed_blob() == b"".join(encs) and len(case.compressed_blob()) == 48 * N
    for i, enc in enumerate(encs):
        back = oracle.p1_uncompress(enc)
        if i in case.inf:
            assert enc == SC.INF_48 and not back.any()
        else:
            assert oracle.p1_equal(back, srs[i]) and oracle.p1_compress(back) == enc


@pytest.mark.parametrize("pattern", ["none", "first", "last", "all"])
def test_file_writer_parses_back(oracle, srs, pattern):
    case = SC.Case(oracle, srs, SC.infinity_set(pattern, N))
    aff = case.affine()
    data = SC.srs_file_bytes(aff)
    assert len(data) == 128 + 96 * N
    f = SC.parse_srs_file(data)
    encs = case.compressed()
    assert f["magic"] == b"KZGSRS1\x00" and f["n"] == N and f["reserved"] == bytes(16)
    assert f["first"] == encs[0] and f["last"] == encs[-1]  # the fingerprints are the oracle's encodings
    assert np.array_equal(f["rows"], aff)
    # the body is x then y, six little-endian 64-bit words each
    i = next((k for k in range(N) if k not in case.inf), None)
    if i is not None:
        x = int.from_bytes(data[128 + 96 * i:128 + 96 * i + 48], "little")
        assert x == SC.row_int(aff[i, :6])
    # overrides reach the header only
    g = SC.parse_srs_file(SC.srs_file_bytes(aff, header_n=5, last=SC.INF_48))
    assert g["n"] == 5 and g["last"] == SC.INF_48 and g["first"] == encs[0] and np.array_equal(g["rows"], aff)
