"""GPU: the producing side on blobs as they travel -- kzg_g1_compress_batch and kzg_fr_to_bytes_batch
against the per-point host encoders; kzg_blobs_to_commitments_bytes / kzg_blobs_to_cells_and_proofs_bytes byte for byte against
(a) the existing entry points chained by hand with every conversion on the host and (b), at the small shapes, tests/blob_oracle.py
with proofs and commitments from the trapdoor oracle, which shares no code with the library; degenerate blobs; every error named;
kzg_recover_cells_and_proofs_bytes against the bytes the blobs produced; the siblings unchanged; threads and multi-device
contexts.  Every test here needs an entry point this change adds."""
import ctypes
import random
import threading

import numpy as np
import pytest

import bigint_twin as T
import blob_oracle as BO
import cells_oracle as CO
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import oracle_ctypes as O
import trapdoor_oracle as TO
import wire_oracle as W

pytestmark = pytest.mark.gpu
R = K.R_MODULUS
S = T.fr_from_be_bytes(T.BENCH_SECRET_BE)
G2 = [K.srs_g2_at(T.BENCH_SECRET_BE, i) for i in range(65)]
INV = K.KZG_ERR_INVALID_ARG
NAT, BRP = K.KZG_ORDER_NATURAL, K.KZG_ORDER_BIT_REVERSED
INF48 = bytes([0xC0]) + bytes(47)
RINV = pow(1 << 256, -1, R)
SHAPES = ((16, 5, 2), (64, 7, 0), (256, 8, 6), (4096, 13, 6), (4096, 12, 6))
SMALL = SHAPES[:3]


@pytest.fixture(scope="module")
def eng():
    e = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(4096)
    yield e
    e.close()


def last(e):
    return K.load_library().kzg_last_error(e._h)


def fails(fn):
    with pytest.raises(K.KzgError) as ei:
        fn()
    return ei.value


def plant(data, width, at, item):
    return data[:width * at] + item + data[width * (at + 1):]


def brp_perm(bits):
    return np.array([CO.brp(i, bits) for i in range(1 << bits)], dtype=np.int64)


def rows_to_be(rows):
    """(count, 4) blst_fr rows -> count x 32 big-endian bytes, on the host"""
    out = bytearray()
    for a, b, c, d in np.asarray(rows, dtype=np.uint64).reshape(-1, 4).tolist():
        out += ((a | b << 64 | c << 128 | d << 192) * RINV % R).to_bytes(32, "big")
    return bytes(out)


def random_blobs(seed, n, batch):
    """batch blobs of n random values, as the n x 32 bytes each travels as (read in either order: the values are random)"""
    rnd = random.Random(seed)
    return [b"".join(rnd.randrange(R).to_bytes(32, "big") for _ in range(n)) for _ in range(batch)]


def blob_of(coeffs, n, order):
    """the bytes of the blob whose polynomial has these coefficients"""
    ev = NO.ntt(list(coeffs) + [0] * (n - len(coeffs)))
    return W.fr_list_be(W.blob_to_spec(ev) if order == BRP else ev)


def route_a(e, blobs, n, K_, t, order):
    """what a caller had to do before: decode, un-permute on the host, kzg_ntt per blob, the batch entry points on coefficient
    arrays, kzg_g1_compress per point, byte swap and spec ordering on the host"""
    lg = n.bit_length() - 1
    M, l = (1 << K_) >> t, 1 << t
    coeffs = []
    for blob in blobs:
        vals = e.fr_from_bytes_batch(blob)
        if order == BRP:
            vals = vals[brp_perm(lg)]
        coeffs.append(e.intt_limbs(vals))
    coms = b"".join(p.compress() for p in e.commit_batch_host(coeffs))
    cells, proofs = e.cells_and_proofs_fk20(np.stack(coeffs), K_, t)
    cm, lm = brp_perm(K_ - t), brp_perm(t)
    out_cells, out_proofs = [], []
    for b in range(len(blobs)):
        v = cells[b].reshape(M, l, 4)
        pr = [p.compress() for p in proofs[b]]
        if order == BRP:  # slot c: this API's cell brp(c), its values in brp order, and that cell's proof
            v = v[cm][:, lm]
            pr = [pr[j] for j in cm]
        out_cells.append(rows_to_be(v))
        out_proofs.append(b"".join(pr))
    return coms, b"".join(out_cells), b"".join(out_proofs)


class Memo:
    def __init__(self):
        self.memo = {}

    def point(self, v):
        if v not in self.memo:
            self.memo[v] = TO.g1_scalar(O, v)
        return self.memo[v]


def route_b(blobs, n, K_, t, order):
    """the byte-level oracle: Python integers only, points as [scalar] G"""
    g = Memo()
    M = (1 << K_) >> t
    coms, cells, proofs = [], [], []
    for blob in blobs:
        c = BO.blob_coefficients(blob, order)
        coms.append(g.point(TO.commitment_scalar(c, S)))
        cells.append(BO.cells_bytes(c, K_, t, order))
        q = TO.cell_proof_scalars_fast(CO.trim(c) or [0], K_, t, S)
        pts = [g.point(q[j]) for j in range(M)]
        proofs.append(b"".join(pts[CO.brp(s, K_ - t)] if order == BRP else pts[s] for s in range(M)))
    return b"".join(coms), b"".join(cells), b"".join(proofs)


# ---- the encoders on their own ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def srs_rows():
    """4097 SRS points as blst_p1 rows rescaled to random Z, infinity not yet planted"""
    rnd = random.Random(1)
    rows = np.asarray(O.srs_g1(4097, T.BENCH_SECRET_BE), dtype=np.uint64).reshape(-1, 18)
    out = []
    for r in rows:
        pt = T.g1_from_blst_p1_limbs([int(x) for x in r])
        assert T.g1_is_on_curve(pt)
        out.append(T.g1_to_blst_p1_limbs(pt, rnd.randrange(1, T.P)))
    return np.array(out, dtype=np.uint64)


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 4097))
def test_g1_compress_batch_equals_the_host_encoder(eng, srs_rows, n):
    rows = srs_rows[:n].copy()
    if n > 2:
        for at in (0, n // 2, n - 1):
            rows[at] = 0
    got = eng.g1_compress_batch(rows)
    assert len(got) == 48 * n
    assert got == b"".join(O.p1_compress(r) for r in rows)
    for at in sorted({0, n // 2, n - 1} & set(range(n))):
        assert got[48 * at:48 * at + 48] == K.G1Point(rows[at]).compress()
    if n > 2:
        assert got[:48] == INF48 and got[-48:] == INF48
    back = eng.g1_uncompress_batch(got)  # the normalised points
    want = np.array([T.g1_to_blst_p1_limbs(T.g1_from_blst_p1_limbs([int(x) for x in r])) for r in rows], dtype=np.uint64)
    assert np.array_equal(back, want.reshape(-1, 18))
    assert eng.g1_compress_batch(back) == got


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 4097))
def test_fr_to_bytes_batch_inverts_fr_from_bytes_batch(eng, n):
    rnd = random.Random(n)
    vals = ([0, 1, R - 1] + [rnd.randrange(R) for _ in range(n)])[:n]
    data = b"".join(W.fr_be_raw(v) for v in vals)
    rows = eng.fr_from_bytes_batch(data)
    assert eng.fr_to_bytes_batch(rows) == data
    assert np.array_equal(eng.fr_from_bytes_batch(eng.fr_to_bytes_batch(rows)), rows)
    if n < 3:
        return
    for image in (R, (1 << 256) - 1):
        for at in (0, n // 2, n - 1):
            bad = rows.copy()
            bad[at] = [(image >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
            ex = fails(lambda: eng.fr_to_bytes_batch(bad))
            assert ex.status == INV and ex.bad_index == at and b"value %d " % at in last(eng) and b"not below r" in last(eng)
    two = rows.copy()
    two[n - 2] = two[1] = [0xFFFFFFFFFFFFFFFF] * 4
    assert fails(lambda: eng.fr_to_bytes_batch(two)).bad_index == 1
    assert eng.fr_to_bytes_batch(rows) == data


# ---- blobs, bit for bit -----------------------------------------------------------------------------------------------------
CASES = [(sh, order, 3, None) for sh in SHAPES for order in (NAT, BRP)] + \
        [((4096, 13, 6), order, batch, None) for order in (NAT, BRP) for batch in (1, 64)] + \
        [((256, 8, 6), BRP, 3, 300), ((16, 5, 2), NAT, 64, 17)]


@pytest.mark.parametrize("shape,order,batch,stride", CASES)
def test_blobs_equal_the_existing_route_and_the_oracle(eng, shape, order, batch, stride):
    n, K_, t = shape
    M = (1 << K_) >> t
    blobs = random_blobs(hash((shape, batch)) & 0xFFFF, n, batch)
    if stride is None:
        data = b"".join(blobs)
    else:  # the blobs lie `stride` values apart, other bytes in between (not even field elements)
        data = b"".join(b + b"\xff" * (32 * (stride - n)) for b in blobs)
    coms, cells, proofs = eng.blobs_to_cells_and_proofs_bytes(data, n, K_, t, order=order, stride=stride)
    assert (len(coms), len(cells), len(proofs)) == (48 * batch, 32 * batch << K_, 48 * batch * M)
    want = route_a(eng, blobs, n, K_, t, order)
    assert coms == want[0]
    assert cells == want[1]
    assert proofs == want[2]
    assert eng.blobs_to_commitments_bytes(data, n, order=order, stride=stride) == coms
    if shape in SMALL and batch == 3:
        assert (coms, cells, proofs) == route_b(blobs, n, K_, t, order)
    if shape == (4096, 13, 6) and order == BRP:  # in spec order the first half of the extension is the blob itself
        for b in range(batch):
            assert cells[32 * b << K_:][:32 * n] == blobs[b]
    # every blob's proofs verify against its commitment, and a flipped byte does not
    for b in range(batch):
        args = (coms[48 * b:48 * b + 48], [0] * M, list(range(M)), cells[32 * b << K_:32 * (b + 1) << K_],
                proofs[48 * M * b:48 * M * (b + 1)], K_, t, G2)
        assert eng.verify_cells_batch_bytes(*args, order=order)
        at = (32 << K_) // 2 + 31
        flipped = args[3][:at] + bytes([args[3][at] ^ 1]) + args[3][at + 1:]
        assert not eng.verify_cells_batch_bytes(*args[:3], flipped, *args[4:], order=order)


def test_commitment_is_that_of_the_evaluations(eng):
    for n in (1, 2, 64, 4096):
        blob = random_blobs(n, n, 1)[0]
        want = eng.commit_evaluations_limbs(eng.fr_from_bytes_batch(blob)).compress()
        assert eng.blobs_to_commitments_bytes(blob, n) == want
        lg = n.bit_length() - 1
        sent = b"".join(blob[32 * j:32 * j + 32] for j in brp_perm(lg))
        assert eng.blobs_to_commitments_bytes(sent, n, order=BRP) == want
    assert eng.blobs_to_commitments_bytes(b"", 64) == b""  # batch = 0


# ---- degenerate blobs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", (NAT, BRP))
def test_degenerate_blobs(eng, order):
    n, K_, t = 64, 7, 2
    M, l = 32, 4
    rnd = random.Random(5)
    zero = bytes(32 * n)
    const = W.fr_be(12345) * n
    short = blob_of([rnd.randrange(R) for _ in range(l)], n, order)  # n' = l: infinity proofs
    shorter = blob_of([0, 7], n, order)
    full = random_blobs(6, n, 2)
    coms, cells, proofs = eng.blobs_to_cells_and_proofs_bytes(zero, n, K_, t, order=order)
    assert coms == INF48 and proofs == INF48 * M and cells == bytes(32 << K_)
    coms, cells, proofs = eng.blobs_to_cells_and_proofs_bytes(const, n, K_, t, order=order)
    assert coms == TO.g1_scalar(O, 12345) and proofs == INF48 * M and cells == W.fr_be(12345) * (1 << K_)
    for blob in (short, shorter):
        coms, cells, proofs = eng.blobs_to_cells_and_proofs_bytes(blob, n, K_, t, order=order)
        assert proofs == INF48 * M
        assert (coms, cells, proofs) == route_b([blob], n, K_, t, order)
    mixed = [full[0], zero, short, const, full[1], shorter]
    got = eng.blobs_to_cells_and_proofs_bytes(b"".join(mixed), n, K_, t, order=order)
    assert got == route_a(eng, mixed, n, K_, t, order)
    assert got == route_b(mixed, n, K_, t, order)
    assert got[2][48 * M:3 * 48 * M] == INF48 * (2 * M) and got[2][:48 * M] != INF48 * M
    # the optional outputs, each left out in turn
    data = b"".join(mixed)
    assert eng.blobs_to_cells_and_proofs_bytes(data, n, K_, t, order=order, commitments=False) == (None,) + got[1:]
    assert eng.blobs_to_cells_and_proofs_bytes(data, n, K_, t, order=order, cells=False) == (got[0], None, got[2])
    assert eng.blobs_to_cells_and_proofs_bytes(data, n, K_, t, order=order, commitments=False, cells=False) == (None, None, got[2])
    # n = 1: a constant over every domain
    one = W.fr_be(99)
    assert eng.blobs_to_cells_and_proofs_bytes(one * 2, 1, 5, 2, order=order) == (TO.g1_scalar(O, 99) * 2, one * 64, INF48 * 16)
    assert eng.blobs_to_cells_and_proofs_bytes(one, 1, 0, 0, order=order) == (TO.g1_scalar(O, 99), one, INF48)
    assert eng.blobs_to_cells_and_proofs_bytes(b"", n, K_, t, order=order) == (b"", b"", b"")


# ---- errors -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", (NAT, BRP))
def test_values_not_below_r_are_named_as_sent(eng, order):
    n, K_, t, batch = 64, 7, 2, 3
    blobs = random_blobs(7, n, batch)
    data = b"".join(blobs)
    good = eng.blobs_to_cells_and_proofs_bytes(data, n, K_, t, order=order)
    for v in (R, (1 << 256) - 1):
        for b, i in ((0, 0), (batch // 2, n // 2), (batch - 1, n - 1)):
            bad = plant(data, 32, b * n + i, W.fr_be_raw(v))
            for call in (lambda: eng.blobs_to_cells_and_proofs_bytes(bad, n, K_, t, order=order),
                         lambda: eng.blobs_to_commitments_bytes(bad, n, order=order)):
                ex = fails(call)
                assert ex.status == INV, (v, b, i)
                assert b"polynomial %d: value %d is not below r" % (b, i) in last(eng), last(eng)
    two = plant(plant(data, 32, 2 * n + 5, W.fr_be_raw(R)), 32, n + 9, W.fr_be_raw(R + 1))
    fails(lambda: eng.blobs_to_commitments_bytes(two, n, order=order))
    assert b"polynomial 1: value 9 " in last(eng)
    assert eng.blobs_to_cells_and_proofs_bytes(data, n, K_, t, order=order) == good  # the context works afterwards


def test_argument_errors(eng):
    n, K_, t = 64, 7, 2
    data = b"".join(random_blobs(8, n, 2))
    assert fails(lambda: eng.blobs_to_commitments_bytes(data, n, order=2)).status == INV and b"order" in last(eng)
    assert fails(lambda: eng.blobs_to_cells_and_proofs_bytes(data, n, K_, t, order=7)).status == INV and b"order" in last(eng)
    assert fails(lambda: eng.blobs_to_commitments_bytes(bytes(32 * 48), 48)).status == INV and b"power of two" in last(eng)
    assert fails(lambda: eng.blobs_to_cells_and_proofs_bytes(bytes(32 * 48), 48, K_, t)).status == INV
    assert fails(lambda: eng.blobs_to_cells_and_proofs_bytes(data, n, 5, 2)).status == INV  # n > N
    assert fails(lambda: eng.blobs_to_cells_and_proofs_bytes(data, n, K_, 7)).status == INV  # log_cell
    lib = K.load_library()
    buf = np.frombuffer(data, dtype=np.uint8)
    out = np.zeros(48 * 4 * 32, dtype=np.uint8)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert lib.kzg_blobs_to_commitments_bytes(eng._h, ptr(buf), n, 2, n - 1, NAT, ptr(out)) == INV and b"stride" in last(eng)
    assert lib.kzg_blobs_to_cells_and_proofs_bytes(eng._h, ptr(buf), n, 2, 32, K_, t, NAT, None, None, ptr(out)) == INV
    assert lib.kzg_blobs_to_commitments_bytes(eng._h, ptr(buf), n, 1, 0, NAT, ptr(out)) == K.KZG_OK  # one blob: stride unused
    assert lib.kzg_blobs_to_commitments_bytes(eng._h, None, n, 2, n, NAT, ptr(out)) == INV and b"NULL" in last(eng)
    assert lib.kzg_blobs_to_commitments_bytes(eng._h, ptr(buf), n, 2, n, NAT, None) == INV
    assert lib.kzg_blobs_to_cells_and_proofs_bytes(eng._h, ptr(buf), n, 2, n, K_, t, NAT, ptr(out), ptr(out), None) == INV
    assert lib.kzg_blobs_to_commitments_bytes(eng._h, None, n, 0, 0, NAT, None) == K.KZG_OK  # batch = 0 does nothing
    bare = K.Engine(0)
    try:
        assert fails(lambda: bare.blobs_to_commitments_bytes(data, n)).status == K.KZG_ERR_NO_SRS
        assert fails(lambda: bare.blobs_to_cells_and_proofs_bytes(data, n, K_, t)).status == K.KZG_ERR_NO_SRS
        assert fails(lambda: bare.blobs_to_commitments_bytes(data, n, order=3)).status == INV  # arguments come first
    finally:
        bare.close()


def test_degree_too_high_names_the_polynomial():
    n, K_, t = 64, 7, 2
    e = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(32)
    try:
        rnd = random.Random(9)
        low = blob_of([rnd.randrange(R) for _ in range(30)], n, NAT)
        edge = blob_of([rnd.randrange(R) for _ in range(36)], n, NAT)  # n' = 36 > 32 points, n' - l = 32 fits
        full = random_blobs(9, n, 1)[0]
        ex = fails(lambda: e.blobs_to_commitments_bytes(low + full + low, n))
        assert ex.status == K.KZG_ERR_DEGREE_TOO_HIGH and b"polynomial 1" in last(e), last(e)
        ex = fails(lambda: e.blobs_to_cells_and_proofs_bytes(low + low + full, n, K_, t, commitments=False))
        assert ex.status == K.KZG_ERR_DEGREE_TOO_HIGH and b"polynomial 2" in last(e), last(e)
        ex = fails(lambda: e.blobs_to_cells_and_proofs_bytes(edge, n, K_, t))
        assert ex.status == K.KZG_ERR_DEGREE_TOO_HIGH and b"polynomial 0" in last(e), last(e)
        for blobs, com in (([low, low], True), ([edge, low], False)):  # blobs of low degree on the same context succeed
            got = e.blobs_to_cells_and_proofs_bytes(b"".join(blobs), n, K_, t, commitments=com)
            want = route_b(blobs, n, K_, t, NAT)
            assert got == ((want[0] if com else None),) + want[1:]
    finally:
        e.close()


# ---- recovery ---------------------------------------------------------------------------------------------------------------
def pick(cells, K_, t, ids, batch):
    """the received rows: slot ids[t] of every polynomial's cells"""
    row = 32 << t
    per = 32 << K_
    return b"".join(cells[b * per + c * row:b * per + (c + 1) * row] for b in range(batch) for c in ids)


@pytest.mark.parametrize("shape,batch", (((4096, 13, 6), 1), ((4096, 13, 6), 8), ((64, 7, 2), 3)))
@pytest.mark.parametrize("order", (NAT, BRP))
def test_recovery_returns_the_bytes_the_blobs_gave(eng, shape, batch, order):
    n, K_, t = shape
    M = (1 << K_) >> t
    data = b"".join(random_blobs(K_ + batch, n, batch))
    _, cells, proofs = eng.blobs_to_cells_and_proofs_bytes(data, n, K_, t, order=order)
    rnd = random.Random(batch)
    shuffled = rnd.sample(range(M), M)
    for name, ids in (("first half", list(range(M // 2))), ("odd", list(range(1, M, 2))), ("random half", shuffled[:M // 2]),
                      ("three quarters", shuffled[:3 * M // 4])):
        got = eng.recover_cells_and_proofs_bytes(n, K_, t, ids, pick(cells, K_, t, ids, batch), order=order)
        assert got[0] == cells, (name, order)
        assert got[1] == proofs, (name, order)
    ids = shuffled[:M // 2]
    recv = pick(cells, K_, t, ids, batch)
    assert eng.recover_cells_and_proofs_bytes(n, K_, t, ids, recv, order=order, proofs=False) == (cells, None)
    assert eng.recover_cells_and_proofs_bytes(n, K_, t, ids, recv, order=order, cells_out=False) == (None, proofs)


@pytest.mark.parametrize("order", (NAT, BRP))
def test_recovery_errors(eng, order):
    n, K_, t, batch = 64, 7, 2, 3
    M, l = 32, 4
    data = b"".join(random_blobs(11, n, batch))
    _, cells, proofs = eng.blobs_to_cells_and_proofs_bytes(data, n, K_, t, order=order)
    ids = random.Random(12).sample(range(M), 24)
    recv = pick(cells, K_, t, ids, batch)
    # a corrupted value: 24 cells over-determine the polynomial
    at = (1 * 24 + 5) * l + 2
    other = W.fr_be((int.from_bytes(recv[32 * at:32 * at + 32], "big") + 1) % R)
    ex = fails(lambda: eng.recover_cells_and_proofs_bytes(n, K_, t, ids, plant(recv, 32, at, other), order=order))
    assert ex.status == K.KZG_ERR_REMAINDER and b"polynomial 1" in last(eng), last(eng)
    for v in (R, (1 << 256) - 1):
        for b, c, i in ((0, 0, 0), (1, 12, 2), (2, 23, 3)):
            bad = plant(recv, 32, (b * 24 + c) * l + i, W.fr_be_raw(v))
            ex = fails(lambda: eng.recover_cells_and_proofs_bytes(n, K_, t, ids, bad, order=order))
            assert ex.status == INV and b"polynomial %d, cell %d: value %d is not below r" % (b, ids[c], i) in last(eng), last(eng)
    ex = fails(lambda: eng.recover_cells_and_proofs_bytes(n, K_, t, ids[:23] + [ids[0]], recv, order=order))
    assert ex.status == INV and b"appears twice" in last(eng)
    ex = fails(lambda: eng.recover_cells_and_proofs_bytes(n, K_, t, ids[:23] + [M], recv, order=order))
    assert ex.status == INV and b"not below N / l" in last(eng)
    assert fails(lambda: eng.recover_cells_and_proofs_bytes(n, K_, t, ids, recv, order=2)).status == INV
    assert fails(lambda: eng.recover_cells_and_proofs_bytes(n, K_, t, ids[:15], pick(cells, K_, t, ids[:15], batch),
                                                            order=order)).status == INV  # k l < n
    bare = K.Engine(0)
    try:
        assert fails(lambda: bare.recover_cells_and_proofs_bytes(n, K_, t, ids, recv, order=order)).status == K.KZG_ERR_NO_SRS
        assert bare.recover_cells_and_proofs_bytes(n, K_, t, ids, recv, order=order, proofs=False) == (cells, None)
    finally:
        bare.close()
    assert eng.recover_cells_and_proofs_bytes(n, K_, t, ids, recv, order=order) == (cells, proofs)


# ---- the siblings, threads, multi-device contexts ---------------------------------------------------------------------------
def test_siblings_are_unchanged_around_a_bytes_call(eng):
    n, K_, t, batch = 4096, 13, 6, 3
    rnd = random.Random(13)
    coeffs = np.stack([K.scalars_to_limbs([rnd.randrange(R) for _ in range(n)]) for _ in range(batch)])
    ids = list(range(0, 128, 2))

    def siblings():
        cells, proofs = eng.cells_and_proofs_fk20(coeffs, K_, t)
        recv = cells.reshape(batch, 128, 64, 4)[:, ids]
        c2, v2, p2 = eng.recover_cells_and_proofs(n, K_, t, ids, recv)
        return cells, np.stack([[p.p1 for p in row] for row in proofs]), c2, v2, np.stack([[p.p1 for p in row] for row in p2])

    before = siblings()
    assert np.array_equal(before[2], coeffs) and np.array_equal(before[3], before[0]) and np.array_equal(before[4], before[1])
    data = b"".join(random_blobs(14, n, 5))
    for order in (NAT, BRP):
        _, cells, proofs = eng.blobs_to_cells_and_proofs_bytes(data, n, K_, t, order=order)
        eng.recover_cells_and_proofs_bytes(n, K_, t, ids, pick(cells, K_, t, ids, 5), order=order)
        after = siblings()
        for a, b in zip(before, after):
            assert np.array_equal(a, b)
    # and the bytes route agrees with them on the same polynomials
    blobs = [rows_to_be(eng.ntt_limbs(c)) for c in coeffs]
    got = eng.blobs_to_cells_and_proofs_bytes(b"".join(blobs), n, K_, t)
    assert got[1] == rows_to_be(before[0]) and got[2] == b"".join(O.p1_compress(r) for r in before[1].reshape(-1, 18))


def test_four_threads_get_the_single_thread_bytes(eng):
    n, K_, t = 4096, 13, 6
    inputs = [(b"".join(random_blobs(20 + i, n, 2 + i)), (NAT, BRP)[i % 2]) for i in range(4)]
    want = [eng.blobs_to_cells_and_proofs_bytes(d, n, K_, t, order=o) for d, o in inputs]
    got, errors = [None] * 4, []

    def work(i):
        try:
            for _ in range(3):
                got[i] = eng.blobs_to_cells_and_proofs_bytes(inputs[i][0], n, K_, t, order=inputs[i][1])
                assert got[i] == want[i]
        except BaseException as ex:  # noqa: BLE001
            errors.append(ex)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert got == want


def test_multi_device_contexts(eng):
    n, K_, t = 64, 7, 2
    data = b"".join(random_blobs(30, n, 3))
    small = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(128)
    try:
        want = {o: small.blobs_to_cells_and_proofs_bytes(data, n, K_, t, order=o) for o in (NAT, BRP)}
    finally:
        small.close()
    ids = list(range(1, 32, 2))
    rep = K.Engine(devices=[0, 0], replicate=True)
    try:
        rep.srs_generate(T.BENCH_SECRET_BE, 128)
        for o in (NAT, BRP):
            assert rep.blobs_to_cells_and_proofs_bytes(data, n, K_, t, order=o) == want[o]
            assert rep.blobs_to_commitments_bytes(data, n, order=o) == want[o][0]
            assert rep.recover_cells_and_proofs_bytes(n, K_, t, ids, pick(want[o][1], K_, t, ids, 3), order=o) == want[o][1:]
        rows = rep.fr_from_bytes_batch(data)
        assert rep.fr_to_bytes_batch(rows) == data
        assert rep.g1_compress_batch(rep.g1_uncompress_batch(want[NAT][2])) == want[NAT][2]
        bad = plant(data, 32, 70, W.fr_be_raw(R))
        assert fails(lambda: rep.blobs_to_commitments_bytes(bad, n)).status == INV and b"polynomial 1: value 6 " in last(rep)
    finally:
        rep.close()
    split = K.Engine(devices=[0, 0])
    try:
        split.srs_generate(T.BENCH_SECRET_BE, 128)
        assert fails(lambda: split.blobs_to_commitments_bytes(data, n)).status == INV and b"range-split" in last(split)
        assert fails(lambda: split.blobs_to_cells_and_proofs_bytes(data, n, K_, t)).status == INV and b"range-split" in last(split)
        ex = fails(lambda: split.recover_cells_and_proofs_bytes(n, K_, t, ids, pick(want[NAT][1], K_, t, ids, 3)))
        assert ex.status == INV and b"range-split" in last(split)
    finally:
        split.close()
