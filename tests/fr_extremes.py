"""Inputs that drive the Fr kernels' lazy sums to the magnitudes their "Bounds" comments allow ("Fr magnitudes
under test").  Pure Python integers; everything is a blst_fr IMAGE (x * 2^256 mod r), which is what the C-ABI carries and
what fr30_from_limbs re-slices into digits: the kernels never see the value behind an image, only the image.

Why r - 1 is not an extreme.  fr30_mul returns the centred residue, and r - 1 = -1 (mod r): after its first product r - 1
is the SMALLEST non-zero magnitude there is.  The largest centred residues are the half values (r -+ 1) / 2, and the
largest digits are those of the digit-extremal images below.

  * half values         H+ = (r - 1) / 2 (centred residue +r/2), H- = (r + 1) / 2 (centred residue -r/2), and neighbours
  * digit-extremal      D+: digits 0..7 all 2^29 - 1 (the largest digit that stays positive), D-: all 2^29 (every digit
                        becomes -2^29 and carries into the next), ALT: the two alternating (the carries make the odd digits
                        +2^29); top digit t = 0 (a small value, its own centred residue) or 0x73ec (just below r)
  * extremal multiplier a point / gamma / weight w reaches the device as the digits of M = w * 2^270 mod r
                        (fr30_arg_from_mont256); multiplier_for(M) is the w whose M is the given image
  * compensated terms   for sum_i m_i c_i with known multipliers: c_i = H / m_i, so every term is congruent to H and all
                        products have one sign, whatever the m_i
  * NTT chain           x[0] = r - 1, x[2^t s] = H for t < m: position 0 of the tile adds +r/2 at each of the m stages
"""
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
R256 = pow(2, 256, R)
R270 = pow(2, 270, R)
H_PLUS = (R - 1) // 2
H_MINUS = (R + 1) // 2
DELTAS = (1, 2, 1 << 30, (1 << 240) + 1)
TOPS = (0, 0x73EC)

NTT_TILE_LOG = 11       # csrc/engine.h: kNttTileLog
NTT_MAX_RADIX_LOG = 9   # kNttMaxRadixLog


def half_values():
    """H+, H- and their neighbours towards the middle of the centred range (all of magnitude just below r / 2)"""
    return [H_PLUS, H_MINUS] + [H_PLUS - d for d in DELTAS] + [H_MINUS + d for d in DELTAS]


def d_plus(t=0):
    return sum(((1 << 29) - 1) << (30 * i) for i in range(8)) + (t << 240)


def d_minus(t=0):
    return sum((1 << 29) << (30 * i) for i in range(8)) + (t << 240)


def d_alt(t=0, first=1):
    """digits 2^29, 2^29 - 1, 2^29, ... (first = 1) or the other phase (first = 0)"""
    return sum(((1 << 29) - (1 if (i + first) % 2 == 0 else 0)) << (30 * i) for i in range(8)) + (t << 240)


def digit_extremal():
    out = []
    for t in TOPS:
        out += [d_plus(t), d_minus(t), d_alt(t, 1), d_alt(t, 0)]
    assert all(0 < v < R for v in out)
    return out


def balanced_digits(v):
    """the nine digits fr30_from_limbs makes of the image v (one parallel carry pass over the unsigned 30-bit slices)"""
    u = [(v >> (30 * i)) & ((1 << 30) - 1) for i in range(8)] + [v >> 240]
    c = [(x + (1 << 29)) >> 30 for x in u[:8]]
    return [u[0] - (c[0] << 30)] + [u[i] - (c[i] << 30) + c[i - 1] for i in range(1, 8)] + [u[8] + c[7]]


def centred(v):
    v %= R
    return v - R if v > R // 2 else v


def multiplier_for(m):
    """the scalar w (a plain value, K.Scalar(w)) that reaches the device as the digits of the integer m: m = w 2^270 mod r"""
    return m % R * pow(R270, -1, R) % R


def multiplier_image_for(m):
    """the same as the blst_fr image of w, for entry points that take the multiplier as limbs"""
    return multiplier_for(m) * R256 % R


def extremal_multipliers():
    """the w whose device form is a half value or a digit-extremal integer"""
    return [multiplier_for(m) for m in (H_PLUS, H_MINUS, d_plus(0), d_minus(0), d_alt(0x73EC), d_plus(0x73EC))]


def compensated(mults, h=H_PLUS):
    """images c_i with c_i m_i = h (mod r) for the plain multipliers m_i (none zero): every term of sum m_i c_i is h"""
    return [h * pow(m % R, -1, R) % R for m in mults]


def ntt_plan(k):
    """the radices of the passes (csrc/ntt_kernels.hip: ntt_plan)"""
    if k <= NTT_TILE_LOG:
        return [k]
    passes = (k + NTT_MAX_RADIX_LOG - 1) // NTT_MAX_RADIX_LOG
    return [k // passes + (1 if i < k % passes else 0) for i in range(passes)]


def ntt_chain(k, h=H_PLUS, partner=None):
    """(x, m): the input of size 2^k whose first pass (radix 2^m, stride s = 2^(k - m)) adds h at every stage to the
    position that starts as r - 1; x as a dict index -> image.  partner: the value at index 2^(m-1) s, which the
    product-free first stage adds as it is (r - 1 there gives the 2 r + (m - 1) r / 2 that canonical inputs can reach at most)"""
    m = ntt_plan(k)[0]
    s = 1 << (k - m)
    x = {0: R - 1}
    for t in range(m):
        x[(1 << t) * s] = h
    if partner is not None and m:
        x[(1 << (m - 1)) * s] = partner
    return x, m


def ntt_chain_small(k, h=H_PLUS, partner=None):
    """the chain seen as a vector of length 2^m (index r for x[r s]): the transform of the full input is periodic with
    period 2^m and equals the transform of this vector, ntt(x)[i] = ntt(small)[i mod 2^m], because w_N^(i r s) = w_(2^m)^(i r)"""
    x, m = ntt_chain(k, h, partner)
    s = 1 << (k - m)
    small = [0] * (1 << m)
    for i, v in x.items():
        small[i // s] = v
    return small, m
