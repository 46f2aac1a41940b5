"""CPU: the host side of blob proofs -- the library's SHA-256 against hashlib at the lengths where the
padding changes, its streaming interface fed in pieces, and kzg_blob_challenges_bytes against tests/blob_proof_oracle.py with
digests in each of [0, r), [r, 2r) and [2r, 2^256), uneven thread shares and padded strides.  The library loads without a GPU."""
import ctypes as C
import hashlib
import random

import numpy as np
import pytest

import blob_proof_oracle as BP
import kzg_poly_commit_exploration_amd as K

R = K.R_MODULUS
INV = K.KZG_ERR_INVALID_ARG
LENGTHS = (0, 1, 55, 56, 63, 64, 65, 119, 120, 128, 131136)  # 55/56, 119/120: the padding takes another block; 131136 =
                                                             # 16 + 16 + 4096 * 32 + 48, a real challenge input


def message(length):
    return random.Random(length).randbytes(length)


@pytest.mark.parametrize("length", LENGTHS)
def test_sha256_equals_hashlib(length):
    m = message(length)
    assert K.sha256(m) == hashlib.sha256(m).digest()


PATHS = (K.KZG_SHA256_PORTABLE, K.KZG_SHA256_SHANI)


def path_or_skip(path):
    if path == K.KZG_SHA256_SHANI and not K.sha256_has_shani():
        pytest.skip("this CPU has no SHA extensions")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("length", LENGTHS)
def test_sha256_on_each_path(length, path):
    path_or_skip(path)
    m = message(length)
    assert K.sha256(m, path=path) == hashlib.sha256(m).digest()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("piece", (1, 63, 64, 65))
@pytest.mark.parametrize("length", LENGTHS)
def test_sha256_streaming_in_pieces(length, piece, path):
    path_or_skip(path)
    m = message(length)
    assert K.sha256(m, piece=piece, path=path) == hashlib.sha256(m).digest()


def test_sha256_path_selection():
    lib = K.load_library()
    out = np.zeros(32, dtype=np.uint8)
    msg = np.frombuffer(b"abc", dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.kzg_sha256_pieces(p(msg), 3, 3, 3, p(out)) == INV and lib.kzg_sha256_pieces(p(msg), 3, 3, -1, p(out)) == INV
    want = 0 if K.sha256_has_shani() else INV  # the extensions are refused where the CPU lacks them, never emulated
    assert lib.kzg_sha256_pieces(p(msg), 3, 3, K.KZG_SHA256_SHANI, p(out)) == want
    assert lib.kzg_sha256_pieces(p(msg), 3, 3, K.KZG_SHA256_AUTO, p(out)) == 0
    assert bytes(out) == hashlib.sha256(b"abc").digest()


def test_sha256_known_answers():
    # FIPS 180-4 examples: "abc" and the 448-bit message
    assert K.sha256(b"abc").hex() == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"
    assert K.sha256(b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq").hex() == \
        "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1"


def fixed_inputs(n, batch, stride, seed=0):
    """batch blobs of n values `stride` values apart with garbage between n and stride, and batch commitments (any bytes:
    they are hashed as given).  Returns (buffer, the blobs, commitments)"""
    rnd = random.Random("blob proofs %d %d %d %d" % (n, batch, stride, seed))
    blobs = [rnd.randbytes(32 * n) for _ in range(batch)]
    buf = b"".join(b + rnd.randbytes(32 * (stride - n)) for b in blobs)
    return buf, blobs, rnd.randbytes(48 * batch)


@pytest.mark.parametrize("pad", (0, 3))
@pytest.mark.parametrize("batch", (1, 3, 20))
@pytest.mark.parametrize("n", (1, 4, 4096))
def test_challenges_equal_the_oracle(n, batch, pad):
    buf, blobs, com = fixed_inputs(n, batch, n + pad)
    got = K.blob_challenges_bytes(buf, n, com, stride=n + pad)
    assert got == BP.challenges_bytes(blobs, com)
    assert all(int.from_bytes(got[32 * b:32 * b + 32], "big") < R for b in range(batch))


def test_challenges_reduce_digests_of_every_range():
    """digests below r, in [r, 2r) and from 2r up: none, one and two subtractions"""
    buf, blobs, com = fixed_inputs(4, 20, 4)
    digests = [BP.digest(b, com[48 * i:48 * i + 48]) for i, b in enumerate(blobs)]
    classes = {min(d // R, 2) for d in digests}
    assert classes == {0, 1, 2}, "the fixed inputs must hold a digest of every range"
    got = K.blob_challenges_bytes(buf, 4, com)
    for i, d in enumerate(digests):
        assert int.from_bytes(got[32 * i:32 * i + 32], "big") == d - (d // R) * R


def test_padding_is_not_hashed_and_the_commitment_is():
    buf, blobs, com = fixed_inputs(4, 3, 6)
    base = K.blob_challenges_bytes(buf, 4, com, stride=6)
    other = bytearray(buf)
    other[32 * 4 + 5] ^= 1  # between n and stride of blob 0
    assert K.blob_challenges_bytes(bytes(other), 4, com, stride=6) == base
    other = bytearray(buf)
    other[32 * 6 + 7] ^= 1  # inside blob 1
    got = K.blob_challenges_bytes(bytes(other), 4, com, stride=6)
    assert got[:32] == base[:32] and got[32:64] != base[32:64] and got[64:] == base[64:]
    c2 = bytearray(com)
    c2[48 * 2 + 47] ^= 1  # one bit of commitment 2
    got = K.blob_challenges_bytes(buf, 4, bytes(c2), stride=6)
    assert got[:64] == base[:64] and got[64:] != base[64:]


def test_argument_errors_and_the_empty_batch():
    lib = K.load_library()
    blob = np.zeros(32 * 8, dtype=np.uint8)
    com = np.zeros(48 * 2, dtype=np.uint8)
    out = np.full(64, 0xAA, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.kzg_blob_challenges_bytes(p(blob), 4, 0, 4, p(com), p(out)) == 0  # batch = 0 does nothing
    assert lib.kzg_blob_challenges_bytes(None, 4, 0, 0, None, None) == 0
    assert bytes(out) == bytes([0xAA]) * 64
    assert lib.kzg_blob_challenges_bytes(None, 4, 1, 4, p(com), p(out)) == INV
    assert lib.kzg_blob_challenges_bytes(p(blob), 4, 1, 4, None, p(out)) == INV
    assert lib.kzg_blob_challenges_bytes(p(blob), 4, 1, 4, p(com), None) == INV
    assert lib.kzg_blob_challenges_bytes(p(blob), 4, 2, 3, p(com), p(out)) == INV  # stride < n with batch > 1
    assert lib.kzg_blob_challenges_bytes(p(blob), 4, 1, 0, p(com), p(out)) == 0    # one blob: the stride is not read
    for n in (0, 3, 6, 1 << (K.KZG_NTT_MAX_LOG + 1)):
        assert lib.kzg_blob_challenges_bytes(p(blob), n, 1, n, p(com), p(out)) == INV
    assert lib.kzg_sha256(None, 1, p(out)) == INV and lib.kzg_sha256(p(blob), 1, None) == INV
    assert lib.kzg_sha256_pieces(p(blob), 1, 0, K.KZG_SHA256_PORTABLE, p(out)) == INV
    assert lib.kzg_sha256(None, 0, p(out)) == 0 and bytes(out[:32]) == hashlib.sha256(b"").digest()
