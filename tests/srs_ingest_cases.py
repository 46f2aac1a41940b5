"""Inputs of the SRS ingest tests (tests/test_srs_ingest_gpu.py), built without the GPU and without the library: every
form in which an SRS reaches the device -- blst_p1 Jacobian rows at a stride, 96-byte affine rows, 48-byte compressed
strings, a KZGSRS1 cache file -- from a list of oracle points and a set of positions that hold the point at infinity.
tests/test_srs_ingest.py checks these builders against the C oracle, so the GPU tests rest on checked inputs.

The geometry the sizes and patterns are chosen for (srs_kernels.hip, srs_io.hip, api.hip):
  * k_normalize            32 consecutive points per lane (kNormK), 64 lanes = 2048 points per workgroup
  * k_uncompress           64 points per workgroup
  * k_affine96_to_table    256 points per workgroup
  * kzg_srs_save           chunks of 65536 points
"""
import random

import numpy as np

import bigint_twin as T

P = T.P
LANE = 32          # srs_kernels.hip kNormK
SAVE_CHUNK = 65536  # api.hip kzg_srs_save
NS = (1, 2, 31, 32, 33, 63, 64, 65, 257, 2047, 2048, 2049, 4097)
FULL_SIZES = (33, 2049)  # every pattern meets every form here
SECRET_BE = T.BENCH_SECRET_BE
MASK64 = (1 << 64) - 1
ONE_ROW = np.array(T.fp_to_mont_limbs(1), dtype=np.uint64)  # Z of a normalised blst_p1

INF_48 = bytes([0xC0]) + bytes(47)
MAGIC = b"KZGSRS1\x00"

# infinity patterns, positions relative to the 32-point lane groups
PATTERNS = ("none", "first", "lane_end", "lane_start", "last", "whole_lane", "all_but_one", "all")


def infinity_set(pattern, n):
    """the positions below n that hold infinity"""
    if pattern == "none":
        s = ()
    elif pattern == "first":
        s = (0,)
    elif pattern == "lane_end":
        s = (LANE - 1,)
    elif pattern == "lane_start":
        s = (LANE,)
    elif pattern == "last":
        s = (n - 1,)
    elif pattern == "whole_lane":  # the second lane's 32 points (what there is of them: the ragged lane at n = 33)
        s = range(LANE, 2 * LANE)
    elif pattern == "all_but_one":  # the survivor sits inside a lane where there is room, neither first nor last
        s = set(range(n)) - {min(n - 1, (2 * n) // 3)}
    elif pattern == "all":
        s = range(n)
    else:
        raise KeyError(pattern)
    return frozenset(i for i in s if 0 <= i < n)


# the patterns tried at each size: all of them at FULL_SIZES, two or three elsewhere, so that every pattern meets three or
# more sizes at which it is not degenerate, small and large ones, besides the full ones
_PATTERNS_AT = {
    1: ("none", "all"),
    2: ("first", "last"),
    31: ("all_but_one", "all"),
    32: ("lane_end", "first"),
    63: ("lane_start", "whole_lane"),
    64: ("whole_lane", "last"),
    65: ("lane_end", "all_but_one"),
    257: ("lane_start", "none"),
    2047: ("last", "first"),
    2048: ("lane_end", "all"),
    4097: ("whole_lane", "all_but_one", "none"),
}


def patterns_for(n):
    return PATTERNS if n in FULL_SIZES else _PATTERNS_AT[n]


# ---- field elements as blst_fp rows ------------------------------------------------------------------------------------------
def fp_row(v):
    """v mod p as blst_fp: 6 x u64 of v * 2^384 mod p"""
    return np.array(T.fp_to_mont_limbs(v % P), dtype=np.uint64)


def raw_row(m):
    """a 384-bit integer as 6 x u64, as it is (no Montgomery conversion, no reduction)"""
    assert 0 <= m < 1 << 384
    return np.array([(m >> (64 * i)) & MASK64 for i in range(6)], dtype=np.uint64)


def row_int(row):
    return sum(int(x) << (64 * i) for i, x in enumerate(row))


TOP_LIMB_LAMBDA = raw_row(0x0123456789ABCDEF << 320)  # only the top limb set, below p's top limb 0x1a0111ea397fe69a
assert row_int(TOP_LIMB_LAMBDA) < P


def lambda_row(kind, rnd):
    """the factor a finite point's Jacobian coordinates are rescaled by, as blst_fp"""
    if kind == 0:
        return fp_row(1)
    if kind == 1:
        return fp_row(P - 1)
    if kind == 2:
        return TOP_LIMB_LAMBDA.copy()
    return fp_row(rnd.randrange(1, P))


# the same few thousand SRS points come back in every case: their encodings and affine rows are computed once
_COMPRESSED = {}
_AFFINE = {}


def _compress_cached(oracle, row):
    key = row.tobytes()
    enc = _COMPRESSED.get(key)
    if enc is None:
        enc = _COMPRESSED[key] = oracle.p1_compress(row)
    return enc


def _affine_cached(enc):
    row = _AFFINE.get(enc)
    if row is None:
        x, y = T.g1_uncompress(enc)
        row = _AFFINE[enc] = np.concatenate([fp_row(x), fp_row(y)])
    return row


# ---- one case: n oracle points, some replaced by infinity ---------------------------------------------------------------------
class Case:
    """points: (n, 18) oracle blst_p1 rows (any Z); inf: the positions that hold infinity instead; seed: for the junk and
    the factors.  Every form below describes the same n points."""

    def __init__(self, oracle, points, inf, seed=0):
        self.oracle = oracle
        self.points = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 18)
        self.n = self.points.shape[0]
        self.inf = frozenset(inf)
        assert all(0 <= i < self.n for i in self.inf)
        self.seed = seed

    # -- 48-byte compressed strings: the oracle's encoding, 0xC0 || 0... for infinity
    def compressed(self):
        return [INF_48 if i in self.inf else _compress_cached(self.oracle, self.points[i]) for i in range(self.n)]

    def compressed_blob(self):
        return b"".join(self.compressed())

    # -- 96-byte affine rows (x, y as blst_fp), (0, 0) = infinity; through Python integers, not the oracle's affine form
    def affine(self):
        out = np.zeros((self.n, 12), dtype=np.uint64)
        for i, enc in enumerate(self.compressed()):
            if i in self.inf:
                continue
            out[i] = _affine_cached(enc)
        return out

    # -- what kzg_srs_read_g1 must give: x, y, Z = Montgomery one; all zero for infinity
    def expected_read(self):
        out = np.zeros((self.n, 18), dtype=np.uint64)
        out[:, :12] = self.affine()
        for i in range(self.n):
            if i not in self.inf:
                out[i, 12:] = ONE_ROW
        return out

    # -- blst_p1 Jacobian rows at a stride of 144 or 432 bytes
    def jacobian(self, stride=144, with_kinds=False, seed=None):
        """finite points rescaled by a seeded factor (1, p - 1, a top-limb-only value, random ones); infinity as Z = 0
        with X, Y left non-zero (what blst leaves behind) or, every other time, all zero; junk in the gap of the stride"""
        assert stride % 8 == 0 and stride >= 144
        seed = self.seed if seed is None else seed
        rnd = random.Random(1000 + seed)
        words = stride // 8
        out = np.zeros((self.n, words), dtype=np.uint64)
        kinds = []
        lib = self.oracle.lib()
        tmp = self.oracle.p1_zeros(1)
        for i in range(self.n):
            if i in self.inf:
                kind = "inf_junk" if (i + seed) % 2 == 0 else "inf_zero"
                if kind == "inf_junk":
                    out[i, :6] = fp_row(rnd.randrange(1, P))
                    out[i, 6:12] = fp_row(rnd.randrange(1, P))
            else:
                kind = (i + seed) % 5  # 0: one, 1: p - 1, 2: top limb only, 3 and 4: random
                lam = np.ascontiguousarray(lambda_row(kind, rnd))
                src = np.ascontiguousarray(self.points[i])
                lib.oracle_p1_rescale(tmp.ctypes.data, src.ctypes.data, lam.ctypes.data)
                out[i, :18] = tmp[0]
            kinds.append(kind)
            for w in range(18, words):
                out[i, w] = rnd.getrandbits(64)
        return (out, kinds) if with_kinds else out


# ---- the KZGSRS1 cache file, written here and not by the library ------------------------------------------------------------------
def affine_row_compress(row):
    """the 48-byte encoding of one 96-byte affine row (through Python integers)"""
    if not np.asarray(row).any():
        return INF_48
    x = T.fp_from_mont_limbs([int(v) for v in row[:6]])
    y = T.fp_from_mont_limbs([int(v) for v in row[6:12]])
    return T.g1_compress((x, y))


def srs_file_bytes(affine_rows, header_n=None, first=None, last=None):
    """128-byte header (magic, n, fingerprints of the first and the last point, 16 reserved bytes) + n x 96 bytes.
    header_n, first, last override what the body says (for the files that must be refused)"""
    rows = np.ascontiguousarray(affine_rows, dtype="<u8").reshape(-1, 12)
    n = rows.shape[0]
    first = affine_row_compress(rows[0]) if first is None else first
    last = affine_row_compress(rows[n - 1]) if last is None else last
    assert len(first) == 48 and len(last) == 48
    header = MAGIC + int(n if header_n is None else header_n).to_bytes(8, "little") + first + last + bytes(16)
    assert len(header) == 128
    return header + rows.tobytes()


def parse_srs_file(data):
    """{'magic', 'n', 'first', 'last', 'reserved', 'rows'}: rows the (len // 96, 12) body, whatever the header claims"""
    assert len(data) >= 128 and (len(data) - 128) % 96 == 0
    return {
        "magic": data[:8],
        "n": int.from_bytes(data[8:16], "little"),
        "first": data[16:64],
        "last": data[64:112],
        "reserved": data[112:128],
        "rows": np.frombuffer(data, dtype="<u8", offset=128).reshape(-1, 12).astype(np.uint64),
    }


# ---- shared, computed once --------------------------------------------------------------------------------------------------------
_SRS = {}


def oracle_srs(oracle, n, secret_be=SECRET_BE):
    """the first n points of the oracle's SRS for the secret (the longest one asked for is kept: shorter ones are its prefix, so ask for the longest first).
    Callers must not write into it"""
    have = _SRS.get(secret_be)
    if have is None or have.shape[0] < n:
        have = oracle.srs_g1(n, secret_be)
        have.setflags(write=False)
        _SRS[secret_be] = have
    return have[:n]


def case(oracle, n, pattern, seed=0):
    return Case(oracle, oracle_srs(oracle, n), infinity_set(pattern, n), seed=seed)
