"""GPU: blob proofs from wire bytes -- kzg_blobs_open_at_bytes, kzg_blobs_to_blob_proofs_bytes and
kzg_verify_blob_proofs_batch_bytes against tests/blob_proof_oracle.py (hashlib, Python integers, proofs as [Q(s)]G for the SRS
of known secret, generated on the device) and, for one shape per quotient path, against the existing entry points byte for byte.
n = 4096 is the last size of the batched quotient kernel, n = 8192 the first of the per-polynomial loop.  Every test here needs
an entry point this change adds."""
import ctypes
import random
import threading

import numpy as np
import pytest

import bigint_twin as T
import blob_oracle as BO
import blob_proof_oracle as BP
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import oracle_ctypes as O
import wire_oracle as W

pytestmark = pytest.mark.gpu
R = K.R_MODULUS
S = T.fr_from_be_bytes(T.BENCH_SECRET_BE)
G2 = [K.srs_g2_at(T.BENCH_SECRET_BE, i) for i in range(2)]
INV = K.KZG_ERR_INVALID_ARG
NAT, BRP = K.KZG_ORDER_NATURAL, K.KZG_ORDER_BIT_REVERSED
INF48 = BP.INF48
SIZES = (1, 2, 4, 64, 4096, 8192)


@pytest.fixture(scope="module")
def eng():
    e = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(8192)
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


def random_blobs(seed, n, batch):
    rnd = random.Random(seed)
    return [b"".join(rnd.randrange(R).to_bytes(32, "big") for _ in range(n)) for _ in range(batch)]


def padded(blobs, n, stride, seed=1):
    """the blobs `stride` values apart, garbage (not below r) in between"""
    rnd = random.Random(seed)
    return b"".join(b + b"\xff" * 32 * (stride - n) if rnd.random() < 0.5 else b + rnd.randbytes(32 * (stride - n)) for b in blobs)


def blob_of(coeffs, n, order):
    ev = NO.ntt(list(coeffs) + [0] * (n - len(coeffs)))
    return W.fr_list_be(W.blob_to_spec(ev) if order == BRP else ev)


_COEF, _OPEN, _COM = {}, {}, {}  # the oracle's results, computed once and shared


def oracle_coefficients(blob, order):
    key = (blob, order)
    if key not in _COEF:
        _COEF[key] = BO.blob_coefficients(blob, order)
    return _COEF[key]


def oracle_open(blob, order, z):
    key = (blob, order, z)
    if key not in _OPEN:
        _OPEN[key] = BP.open_at(O, blob, order, z, S, coeffs=oracle_coefficients(blob, order))
    return _OPEN[key]


def oracle_commitment(blob, order):
    key = (blob, order)
    if key not in _COM:
        _COM[key] = BP.commitment(O, blob, order, S, coeffs=oracle_coefficients(blob, order))
    return _COM[key]


def zs_bytes(zs):
    return b"".join(z.to_bytes(32, "big") for z in zs)


# ---- kzg_blobs_open_at_bytes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", (NAT, BRP))
@pytest.mark.parametrize("batch", (1, 3))
@pytest.mark.parametrize("n", SIZES)
def test_open_at_equals_the_oracle(eng, n, batch, order):
    rnd = random.Random(n * 10 + batch)
    blobs = random_blobs(n + batch, n, batch)
    zs = [rnd.randrange(R) for _ in range(batch)]  # a point of its own per polynomial
    stride = n + 3
    want = [oracle_open(b, order, z) for b, z in zip(blobs, zs)]
    for data, st in ((b"".join(blobs), None), (padded(blobs, n, stride), stride)):
        ys, proofs = eng.blobs_open_at_bytes(data, n, zs_bytes(zs), order=order, stride=st)
        assert ys == b"".join(w[0] for w in want), (n, batch, st)
        assert proofs == b"".join(w[1] for w in want), (n, batch, st)
    if n == 1:
        assert proofs == INF48 * batch and ys == b"".join(blobs)


def test_open_at_with_uneven_msm_sub_batches():
    """batch 5 with at most 2 polynomials per MSM: sub-batches of 2, 2 and 1"""
    e = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(64)
    try:
        assert e.set_max_batch(2) == 2
        for n, order in ((64, NAT), (4, BRP)):
            blobs = random_blobs(50 + n, n, 5)
            zs = [random.Random(n + i).randrange(R) for i in range(5)]
            want = [oracle_open(b, order, z) for b, z in zip(blobs, zs)]
            ys, proofs = e.blobs_open_at_bytes(b"".join(blobs), n, zs_bytes(zs), order=order)
            assert ys == b"".join(w[0] for w in want) and proofs == b"".join(w[1] for w in want)
            coms, prf = e.blobs_to_blob_proofs_bytes(b"".join(blobs), n, order=order)
            assert coms == b"".join(oracle_commitment(b, order) for b in blobs)
            cz = [BP.challenge(b, coms[48 * i:48 * i + 48]) for i, b in enumerate(blobs)]
            assert prf == b"".join(oracle_open(b, order, z)[1] for b, z in zip(blobs, cz))
            assert e.verify_blob_proofs_batch_bytes(b"".join(blobs), n, coms, prf, G2, order=order)
    finally:
        e.close()


@pytest.mark.parametrize("n", (4096, 8192))
def test_open_at_equals_the_existing_entry_points(eng, n):
    """one shape per quotient path: y is kzg_evaluate_evaluations_batch's, the proof kzg_g1_compress(kzg_open_evaluations(...))"""
    batch = 3
    blobs = random_blobs(7 * n, n, batch)
    zs = [random.Random(n + i).randrange(R) for i in range(batch)]
    ys, proofs = eng.blobs_open_at_bytes(b"".join(blobs), n, zs_bytes(zs))
    vals = eng.fr_from_bytes_batch(b"".join(blobs)).reshape(batch, n, 4)
    want_ys = eng.evaluate_evaluations_batch(vals, [K.Scalar(z) for z in zs])
    assert ys == b"".join(W.fr_be(int(y.v)) for y in want_ys)
    for b in range(batch):
        p = eng.open_evaluations_limbs(vals[b], K.Scalar(zs[b]), want_ys[b])
        assert proofs[48 * b:48 * b + 48] == p.compress()


@pytest.mark.parametrize("order", (NAT, BRP))
@pytest.mark.parametrize("n", (4, 64, 4096, 8192))
def test_open_at_special_points(eng, n, order):
    lg = n.bit_length() - 1
    w = NO.domain_root(lg)
    k = n // 2 + 1 if n > 4 else 2  # an interior domain point
    points = [0, R - 1, 1, pow(w, n - 1, R), pow(w, k, R)]
    index = [None, None, 0, n - 1, k]
    blob = random_blobs(3 * n + order, n, 1)[0]
    data = blob * len(points)
    ys, proofs = eng.blobs_open_at_bytes(data, n, zs_bytes(points), order=order)
    sent = [blob[32 * i:32 * i + 32] for i in range(n)]
    for j, (z, i) in enumerate(zip(points, index)):
        want = oracle_open(blob, order, z)
        assert ys[32 * j:32 * j + 32] == want[0] and proofs[48 * j:48 * j + 48] == want[1], (n, z)
        if i is not None:  # inside the domain: the blob's own value there (value i of this API sits at brp(i) as sent)
            at = int(format(i, "0%db" % lg)[::-1], 2) if order == BRP else i
            assert ys[32 * j:32 * j + 32] == sent[at], (n, i)


@pytest.mark.parametrize("order", (NAT, BRP))
def test_open_at_degenerate_blobs(eng, order):
    for n in (64, 8192):
        zero = bytes(32 * n)
        const = W.fr_be(12345) * n
        full = random_blobs(n, n, 1)[0]
        z = [5, 6, 7, 8]
        ys, proofs = eng.blobs_open_at_bytes(const + full + zero + const, n, zs_bytes(z), order=order)
        assert proofs[:48] == INF48 and proofs[96:] == INF48 * 2 and proofs[48:96] == oracle_open(full, order, 6)[1]
        assert ys[:32] == W.fr_be(12345) and ys[64:96] == bytes(32) and ys[96:] == W.fr_be(12345)
        ys, proofs = eng.blobs_open_at_bytes(const + zero, n, zs_bytes(z[:2]), order=order)  # nothing for the MSM to do
        assert proofs == INF48 * 2 and ys == W.fr_be(12345) + bytes(32)
    assert eng.blobs_open_at_bytes(b"", 64, b"", order=order) == (b"", b"")  # batch = 0


def test_open_at_with_a_short_srs():
    n = 64
    e = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(32)
    try:
        rnd = random.Random(9)
        low = blob_of([rnd.randrange(R) for _ in range(30)], n, NAT)
        edge = blob_of([rnd.randrange(R) for _ in range(33)], n, NAT)  # n' - 1 = 32 fits the proof, n' = 33 no commitment
        over = blob_of([rnd.randrange(R) for _ in range(34)], n, NAT)  # n' - 1 = 33 > 32 points
        zs = [11, 12, 13]
        ys, proofs = e.blobs_open_at_bytes(low + edge + low, n, zs_bytes(zs))
        want = [oracle_open(b, NAT, z) for b, z in zip((low, edge, low), zs)]
        assert ys == b"".join(w[0] for w in want) and proofs == b"".join(w[1] for w in want)
        ex = fails(lambda: e.blobs_open_at_bytes(low + low + over, n, zs_bytes(zs)))
        assert ex.status == K.KZG_ERR_DEGREE_TOO_HIGH and b"polynomial 2" in last(e), last(e)
        ex = fails(lambda: e.blobs_to_blob_proofs_bytes(low + edge + low, n))  # the commitment of polynomial 1 needs 33 points
        assert ex.status == K.KZG_ERR_DEGREE_TOO_HIGH and b"polynomial 1" in last(e), last(e)
        coms = b"".join(oracle_commitment(b, NAT) for b in (low, edge, low))
        got = e.blobs_to_blob_proofs_bytes(low + edge + low, n, commitments48=coms)  # given: no commitment MSM
        cz = [BP.challenge(b, coms[48 * i:48 * i + 48]) for i, b in enumerate((low, edge, low))]
        assert got == (coms, b"".join(oracle_open(b, NAT, z)[1] for b, z in zip((low, edge, low), cz)))
    finally:
        e.close()


@pytest.mark.parametrize("order", (NAT, BRP))
def test_open_at_errors(eng, order):
    n, batch = 64, 3
    blobs = random_blobs(21, n, batch)
    data = b"".join(blobs)
    zs = zs_bytes([3, 4, 5])
    good = eng.blobs_open_at_bytes(data, n, zs, order=order)
    for v in (R, (1 << 256) - 1):
        for i in (0, n - 1):  # the first and the last position of the last polynomial, named as sent
            bad = plant(data, 32, (batch - 1) * n + i, W.fr_be_raw(v))
            for call in (lambda: eng.blobs_open_at_bytes(bad, n, zs, order=order),  # noqa: B023
                         lambda: eng.blobs_to_blob_proofs_bytes(bad, n, order=order)):  # noqa: B023
                ex = fails(call)
                assert ex.status == INV and b"polynomial %d: value %d is not below r" % (batch - 1, i) in last(eng), last(eng)
        ex = fails(lambda: eng.blobs_open_at_bytes(data, n, plant(zs, 32, 1, W.fr_be_raw(v)), order=order))  # noqa: B023
        assert ex.status == INV and b"polynomial 1: the point z is not below r" in last(eng), last(eng)
    assert fails(lambda: eng.blobs_open_at_bytes(data, n, zs, order=2)).status == INV and b"order" in last(eng)
    assert fails(lambda: eng.blobs_open_at_bytes(bytes(32 * 48), 48, zs[:32])).status == INV and b"power of two" in last(eng)
    lib = K.load_library()
    buf = np.frombuffer(data, dtype=np.uint8)
    zb = np.frombuffer(zs, dtype=np.uint8)
    out = np.zeros(48 * 4, dtype=np.uint8)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert lib.kzg_blobs_open_at_bytes(eng._h, ptr(buf), n, 2, n - 1, order, ptr(zb), ptr(out), ptr(out)) == INV and b"stride" in last(eng)
    assert lib.kzg_blobs_open_at_bytes(eng._h, None, n, 2, n, order, ptr(zb), ptr(out), ptr(out)) == INV and b"NULL" in last(eng)
    assert lib.kzg_blobs_open_at_bytes(eng._h, ptr(buf), n, 2, n, order, None, ptr(out), ptr(out)) == INV
    assert lib.kzg_blobs_open_at_bytes(eng._h, ptr(buf), n, 2, n, order, ptr(zb), None, ptr(out)) == INV
    assert lib.kzg_blobs_open_at_bytes(eng._h, ptr(buf), n, 2, n, order, ptr(zb), ptr(out), None) == INV
    assert lib.kzg_blobs_to_blob_proofs_bytes(eng._h, ptr(buf), n, 2, n, order, None, None, None) == INV
    assert lib.kzg_blobs_open_at_bytes(eng._h, None, n, 0, 0, order, None, None, None) == K.KZG_OK  # batch = 0 does nothing
    assert lib.kzg_blobs_to_blob_proofs_bytes(eng._h, None, n, 0, 0, order, None, None, None) == K.KZG_OK
    bare = K.Engine(0)
    try:
        assert fails(lambda: bare.blobs_open_at_bytes(data, n, zs, order=order)).status == K.KZG_ERR_NO_SRS
        assert fails(lambda: bare.blobs_to_blob_proofs_bytes(data, n, order=order)).status == K.KZG_ERR_NO_SRS
        assert fails(lambda: bare.blobs_open_at_bytes(data, n, zs, order=3)).status == INV  # arguments come first
    finally:
        bare.close()
    assert eng.blobs_open_at_bytes(data, n, zs, order=order) == good  # the context works afterwards


# ---- kzg_blobs_to_blob_proofs_bytes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", (NAT, BRP))
@pytest.mark.parametrize("n,batch", ((1, 3), (4, 1), (64, 3), (4096, 3), (8192, 1)))
def test_blob_proofs_with_and_without_given_commitments(eng, n, batch, order):
    blobs = random_blobs(31 * n + batch, n, batch)
    stride = n + 2
    data = padded(blobs, n, stride)
    want_coms = eng.blobs_to_commitments_bytes(data, n, order=order, stride=stride)
    assert want_coms == b"".join(oracle_commitment(b, order) for b in blobs)
    cz = zs_bytes([BP.challenge(b, want_coms[48 * i:48 * i + 48]) for i, b in enumerate(blobs)])
    assert K.blob_challenges_bytes(data, n, want_coms, stride=stride) == cz
    _, want_proofs = eng.blobs_open_at_bytes(data, n, cz, order=order, stride=stride)
    assert eng.blobs_to_blob_proofs_bytes(data, n, order=order, stride=stride) == (want_coms, want_proofs)
    assert eng.blobs_to_blob_proofs_bytes(data, n, commitments48=want_coms, order=order, stride=stride) == (want_coms, want_proofs)
    if n > 1:
        other = bytearray(want_coms)
        other[48 * (batch - 1) + 20] ^= 4  # one bit of the last commitment: another challenge, another proof
        got = eng.blobs_to_blob_proofs_bytes(data, n, commitments48=bytes(other), order=order, stride=stride)
        assert got[0] == bytes(other)
        assert got[1][:48 * (batch - 1)] == want_proofs[:48 * (batch - 1)] and got[1][48 * (batch - 1):] != want_proofs[48 * (batch - 1):]


# ---- kzg_verify_blob_proofs_batch_bytes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", (NAT, BRP))
@pytest.mark.parametrize("n,batch", ((64, 1), (64, 5), (4096, 5)))
def test_verify_blob_proofs(eng, n, batch, order):
    blobs = random_blobs(41 * n + batch, n, batch)
    data = b"".join(blobs)
    coms, proofs = eng.blobs_to_blob_proofs_bytes(data, n, order=order)
    cz = zs_bytes([BP.challenge(b, coms[48 * i:48 * i + 48]) for i, b in enumerate(blobs)])

    def both(d, c, p):
        """the verdict, which must be kzg_verify_blobs_batch_bytes's at the oracle's points for the same inputs"""
        z = zs_bytes([BP.challenge(d[32 * n * i:32 * n * (i + 1)], c[48 * i:48 * i + 48]) for i in range(batch)])
        got = eng.verify_blob_proofs_batch_bytes(d, n, c, p, G2, order=order)
        assert got == eng.verify_blobs_batch_bytes(d, n, c, z, p, G2, order=order, want_ys=False)[0]
        return got

    assert both(data, coms, proofs)
    assert eng.verify_blobs_batch_bytes(data, n, coms, cz, proofs, G2, order=order, want_ys=False)[0]
    at = 32 * n * (batch - 1) + 32 * (n // 2) + 31
    flipped = data[:at] + bytes([data[at] ^ 1]) + data[at + 1:]  # one byte of one blob
    assert not both(flipped, coms, proofs)
    if batch > 1:
        swapped = proofs[48:96] + proofs[:48] + proofs[96:]  # two proofs swapped
        assert not both(data, coms, swapped)
        replaced = coms[:48] + coms[:48] + coms[96:]  # commitment 1 replaced by blob 0's
        assert not both(data, replaced, proofs)
    # the sibling's errors in the sibling's words
    bad = plant(data, 32, n * (batch - 1) + 3, W.fr_be_raw(R))
    ex = fails(lambda: eng.verify_blob_proofs_batch_bytes(bad, n, coms, proofs, G2, order=order))
    msg = last(eng)
    ex2 = fails(lambda: eng.verify_blobs_batch_bytes(bad, n, coms, cz, proofs, G2, order=order))
    assert ex.status == ex2.status == INV and msg == last(eng) and b"is not below r" in msg, msg
    ex = fails(lambda: eng.verify_blob_proofs_batch_bytes(data, n, coms, proofs, G2, order=5))
    msg = last(eng)
    fails(lambda: eng.verify_blobs_batch_bytes(data, n, coms, cz, proofs, G2, order=5))
    assert ex.status == INV and msg == last(eng) and b"order" in msg
    assert eng.verify_blob_proofs_batch_bytes(b"", n, b"", b"", G2, order=order)  # batch = 0: nothing to refute


# ---- threads --------------------------------------------------------------------------------------------------------------------
def test_two_threads_get_the_right_bytes(eng):
    n = 4096
    inputs = [(b"".join(random_blobs(60 + i, n, 2 + i)), (NAT, BRP)[i]) for i in range(2)]
    want = [eng.blobs_to_blob_proofs_bytes(d, n, order=o) for d, o in inputs]
    for (d, o), (coms, proofs) in zip(inputs, want):
        assert eng.verify_blob_proofs_batch_bytes(d, n, coms, proofs, G2, order=o)
        assert coms == eng.blobs_to_commitments_bytes(d, n, order=o)
    got, errors = [None] * 2, []

    def work(i):
        try:
            for _ in range(3):
                got[i] = eng.blobs_to_blob_proofs_bytes(inputs[i][0], n, order=inputs[i][1])
                assert got[i] == want[i]
        except BaseException as ex:  # noqa: BLE001
            errors.append(ex)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert got == want


def test_multi_device_contexts():
    n = 64
    blobs = random_blobs(70, n, 3)
    data = b"".join(blobs)
    zs = zs_bytes([9, 10, 11])
    want = [oracle_open(b, NAT, z) for b, z in zip(blobs, (9, 10, 11))]
    rep = K.Engine(devices=[0, 0], replicate=True)
    try:
        rep.srs_generate(T.BENCH_SECRET_BE, 128)
        assert rep.blobs_open_at_bytes(data, n, zs) == (b"".join(w[0] for w in want), b"".join(w[1] for w in want))
        coms, proofs = rep.blobs_to_blob_proofs_bytes(data, n)
        assert coms == b"".join(oracle_commitment(b, NAT) for b in blobs)
        assert rep.verify_blob_proofs_batch_bytes(data, n, coms, proofs, G2)
    finally:
        rep.close()
    split = K.Engine(devices=[0, 0])
    try:
        split.srs_generate(T.BENCH_SECRET_BE, 128)
        assert fails(lambda: split.blobs_open_at_bytes(data, n, zs)).status == INV and b"range-split" in last(split)
        assert fails(lambda: split.blobs_to_blob_proofs_bytes(data, n)).status == INV and b"range-split" in last(split)
    finally:
        split.close()
