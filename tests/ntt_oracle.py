"""Independent references for the NTT entry points (kzg_ntt, kzg_commit_evaluations, kzg_open_evaluations), in Python
integers mod r.

Domain of size n = 2^k: {w^i}, w = 7^((r - 1) / n), natural order on both sides: ntt(c)[i] = P(w^i) for P = sum c_j X^j.
  * ntt / intt        iterative radix-2 transforms (bit-reversal permutation, then Cooley-Tukey stages)
  * dft               the O(n^2) definition, for checking the fast transform at small n
  * barycentric_eval  P(s) straight from the values: (s^n - 1) / n * sum_i e_i w^i / (s - w^i), s outside the domain;
                      no transform, so it checks a commitment from evaluations against [P(s)]G on its own
"""
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
GENERATOR = 7
TWO_ADICITY = 32


def domain_root(k):
    assert 0 <= k <= TWO_ADICITY
    return pow(GENERATOR, (R - 1) >> k, R)


def log2_exact(n):
    k = n.bit_length() - 1
    assert n >= 1 and n == 1 << k, n
    return k


def _transform(vals, w):
    n = len(vals)
    k = log2_exact(n)
    a = [0] * n
    for i, v in enumerate(vals):  # bit-reversed order
        j = int(format(i, "0%db" % k)[::-1], 2) if k else 0
        a[j] = v % R
    h = 1
    while h < n:
        wh = pow(w, n // (2 * h), R)
        tw = [1] * h
        for i in range(1, h):
            tw[i] = tw[i - 1] * wh % R
        for start in range(0, n, 2 * h):
            for i in range(h):
                x = a[start + i]
                y = a[start + i + h] * tw[i] % R
                a[start + i] = (x + y) % R
                a[start + i + h] = (x - y) % R
        h *= 2
    return a


def ntt(coeffs):
    """coefficients -> values over the domain"""
    return _transform(coeffs, domain_root(log2_exact(len(coeffs))))


def intt(evals):
    """values over the domain -> coefficients"""
    n = len(evals)
    w = domain_root(log2_exact(n))
    inv_n = pow(n, R - 2, R)
    return [v * inv_n % R for v in _transform(evals, pow(w, R - 2, R))]


def dft(vals, inverse=False):
    n = len(vals)
    w = domain_root(log2_exact(n))
    if inverse:
        w = pow(w, R - 2, R)
    out = [sum(v * pow(w, i * j, R) for j, v in enumerate(vals)) % R for i in range(n)]
    if inverse:
        inv_n = pow(n, R - 2, R)
        out = [v * inv_n % R for v in out]
    return out


def batch_inverse(vals):
    """1 / v for every v (none zero): one inversion, 3 (n - 1) products"""
    prefix = [1] * (len(vals) + 1)
    for i, v in enumerate(vals):
        prefix[i + 1] = prefix[i] * v % R
    inv = pow(prefix[-1], R - 2, R)
    out = [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = prefix[i] * inv % R
        inv = inv * vals[i] % R
    return out


def barycentric_eval(evals, s):
    """P(s) for the P of degree < n with P(w^i) = evals[i]; s inside the domain returns the matching value"""
    n = len(evals)
    w = domain_root(log2_exact(n))
    s %= R
    pts = [1] * n
    for i in range(1, n):
        pts[i] = pts[i - 1] * w % R
    for i, p in enumerate(pts):
        if p == s:
            return evals[i] % R
    inv = batch_inverse([(s - p) % R for p in pts])
    acc = 0
    for e, p, d in zip(evals, pts, inv):
        acc = (acc + e * p % R * d) % R
    return (pow(s, n, R) - 1) * pow(n, R - 2, R) % R * acc % R
