"""Byte-level restatement of the producing side, for the tests: blob bytes -> values -> coefficients
-> cells, and the bytes every output travels as.  Everything here is Python integers over oracle/bigint_twin.py,
ntt_oracle, cells_oracle and wire_oracle; nothing of the library is used."""
import bigint_twin as T
import cells_oracle as CO
import ntt_oracle as NO
import wire_oracle as W

R = T.R
NATURAL, BIT_REVERSED = 0, 1


def blob_values(blob_be, order):
    """the n evaluations over the n-domain in this API's (natural) order"""
    assert len(blob_be) % 32 == 0
    vals = [int.from_bytes(blob_be[32 * i:32 * i + 32], "big") for i in range(len(blob_be) // 32)]
    assert all(v < R for v in vals)
    return W.blob_to_spec(vals) if order == BIT_REVERSED else vals  # brp is an involution


def blob_coefficients(blob_be, order):
    return NO.intt(blob_values(blob_be, order))


def cells_bytes(coeffs, K, t, order):
    """the N values of all cells as they leave: cell-major, or the specs' order (slot c = this API's cell brp(c), values in
    brp order)"""
    M, l = (1 << K) >> t, 1 << t
    v = CO.cells(list(coeffs), K, t)
    rows = [v[j * l:(j + 1) * l] for j in range(M)]
    if order == BIT_REVERSED:
        rows = [W.cells_to_spec([CO.brp(c, K - t)], [rows[CO.brp(c, K - t)]], K, t)[1][0] for c in range(M)]
    return b"".join(W.fr_list_be(r) for r in rows)


def proofs_bytes(points, K, t, order):
    """M proof points (this API's numbering) -> M x 48 bytes in the order asked"""
    M = (1 << K) >> t
    assert len(points) == M
    if order == BIT_REVERSED:
        points = [points[CO.brp(c, K - t)] for c in range(M)]
    return b"".join(T.g1_compress(p) for p in points)
