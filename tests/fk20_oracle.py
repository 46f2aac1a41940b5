"""Fr shadow of the FK20 route of kzg_cells_and_proofs_fk20 (csrc/fk20_kernels.hip), in Python
integers mod r: a G1 point [x]G is stood in for by x, so every G1 DFT becomes an Fr DFT and the proofs come out as the
scalars q_j(s) that the proofs are multiples of G by.

Domain of N = 2^K points, cells of l = 2^t, n' coefficients (trailing zeros dropped), m = ceil(n'/l), L the smallest power of
two >= 2m, M = N/l cells.  With a_j = w_N^(j l) = w_M^j:
    q_j(s) = sum_{d=0}^{m-2} a_j^d H_d,   H_d = sum_i c_(i + (d+1) l) s^i,
so (q_j(s))_j = DFT_M(H_0, .., H_(m-2), 0, ..).  The H_d are l Toeplitz products by circulant embedding:
    conv = IDFT_L( sum_r DFT_L(S_r) . DFT_L(R_r) ),   H_d = conv[m - 1 - d],
    R_r[k] = c_((m - k) l + r) for 1 <= k <= m, zero elsewhere.
S_r comes in two forms: the issue's, S_r[v] = s^(v l + r) for v < m and v l + r < n' - l (zero elsewhere), and the
library's cached one, S_r[v] = s^(v l + r) for v < L/2 and v l + r inside the SRS: it does not depend on n', and the
extra entries only ever meet zeros of R_r in the outputs that are read."""
import cells_oracle as CO
import ntt_oracle as NO

R = NO.R


def shape(n_eff, t):
    """(l, m, L) for n' coefficients and cells of 2^t points"""
    l = 1 << t
    m = -(-n_eff // l)
    L = 1
    while L < 2 * m:
        L <<= 1
    return l, m, L


def srs_side(s_pows, n_eff, t, cached):
    """S_r for r < l as lists of L scalars; s_pows[i] = s^i for every SRS point"""
    l, m, L = shape(n_eff, t)
    out = []
    for r in range(l):
        if cached:
            S = [s_pows[v * l + r] if v < L // 2 and v * l + r < len(s_pows) else 0 for v in range(L)]
        else:
            S = [s_pows[v * l + r] if v < m and v * l + r < n_eff - l else 0 for v in range(L)]
        out.append(S)
    return out


def toeplitz_h(vals, t, s_pows, cached=True):
    """H_0 .. H_(m-2) by the circulant embedding"""
    c = CO.trim(vals)
    n_eff = len(c)
    l, m, L = shape(n_eff, t)
    acc = [0] * L
    for r, S in enumerate(srs_side(s_pows, n_eff, t, cached)):
        Rr = [c[(m - k) * l + r] if 1 <= k <= m and (m - k) * l + r < n_eff else 0 for k in range(L)]
        A, B = NO.ntt(Rr), NO.ntt(S)
        acc = [(x + a * b) % R for x, a, b in zip(acc, A, B)]
    conv = NO.intt(acc)
    return [conv[m - 1 - d] for d in range(m - 1)]


def toeplitz_h_direct(vals, t, s):
    """H_d = sum_i c_(i + (d+1) l) s^i, straight from the definition"""
    c = CO.trim(vals)
    l = 1 << t
    m = -(-len(c) // l)
    return [sum(c[i + (d + 1) * l] * pow(s, i, R) for i in range(len(c) - (d + 1) * l)) % R for d in range(m - 1)]


def fk20_proof_scalars(vals, K, t, s_pows, cached=True):
    """the N/l proofs' scalars by FK20: DFT_(N/l) of the H_d zero-padded"""
    c = CO.trim(vals)
    M = (1 << K) >> t
    if len(c) <= (1 << t):
        return [0] * M
    H = toeplitz_h(c, t, s_pows, cached)
    assert len(H) <= M
    return NO.ntt(H + [0] * (M - len(H)))


def cell_proof_scalars(vals, K, t, s):
    """the same from the stride-l synthetic division of every cell (what kzg_cells_and_proofs commits to)"""
    M = (1 << K) >> t
    return [CO.poly_eval(CO.stride_quotient(vals, 1 << t, CO.cell_root(K, t, j)), s) for j in range(M)]
