"""Restatement of blob proofs and their Fiat-Shamir challenges, for the tests: the challenge with
hashlib, y from the interpolated coefficients, the proof as [(P(s) - y) / (s - z)] G for an SRS of known secret.  Python integers
over blob_oracle and trapdoor_oracle; nothing of the library is used."""
import hashlib

import bigint_twin as T
import blob_oracle as BO
import trapdoor_oracle as TO

R = T.R
DOMAIN = b"FSBLOBVERIFY_V1_"
INF48 = bytes([0xC0]) + bytes(47)


def digest(blob_be, commitment48):
    """the 256-bit integer the challenge is reduced from; blob_be: the n x 32 bytes as sent"""
    assert len(blob_be) % 32 == 0 and len(commitment48) == 48
    n = len(blob_be) // 32
    return int.from_bytes(hashlib.sha256(DOMAIN + n.to_bytes(16, "big") + bytes(blob_be) + bytes(commitment48)).digest(), "big")


def challenge(blob_be, commitment48):
    return digest(blob_be, commitment48) % R


def challenges_bytes(blobs, commitments48):
    """blobs: a list of byte strings; commitments48: batch x 48 bytes -> batch x 32 big-endian bytes"""
    return b"".join(challenge(b, commitments48[48 * i:48 * i + 48]).to_bytes(32, "big") for i, b in enumerate(blobs))


def open_at(oracle, blob_be, order, z, s, coeffs=None):
    """(y as 32 big-endian bytes, the 48 proof bytes) of the blob's polynomial at z, for the SRS of secret s; coeffs: the blob's
    coefficients when the caller has them already (blob_oracle.blob_coefficients)"""
    c = BO.blob_coefficients(blob_be, order) if coeffs is None else coeffs
    y = TO.poly_eval(c, z)
    q = TO.proof_scalar(c, z, s, y)
    return y.to_bytes(32, "big"), (TO.g1_scalar(oracle, q) if q else INF48)


def commitment(oracle, blob_be, order, s, coeffs=None):
    v = TO.commitment_scalar(BO.blob_coefficients(blob_be, order) if coeffs is None else coeffs, s)
    return TO.g1_scalar(oracle, v) if v else INF48
