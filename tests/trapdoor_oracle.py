"""Independent references for the boundary tests (tests/test_msm_boundaries_gpu.py, tests/test_scan_points_gpu.py).

Trapdoor oracle: with the secret s of the trusted setup known, every group element the library computes is [v]G for a
scalar v that O(n) work in Python integers mod r gives -- no MSM, so adversarial inputs can be checked at 2^20 and 2^22
terms in seconds:
  * commitment  [P(s)]G
  * proof       [(P(s) - y) / (s - z)]G             (s = z: [P'(z)]G, the quotient's value there)
  * multiproof  [(P(s) - I(s)) / Z(s)]G              I the interpolant of the claims, Z = prod (X - z_i)
  * cell proof  [(P(s) - I_j(s)) / (s^l - a_j)]G       one per cell of a domain (s^l = a_j: the stride quotient at s)
  * G1 DFT      of the SRS [s^i]G: [(s^m - 1) / (s w^j - 1)]G   (s w^j = 1: [m]G)
The only group operation is one scalar multiplication of the generator by the C oracle (oracle_p1_mult).

Torsion: points of each small prime order of the G1 cofactor h1, for the subgroup checks of the verifier
(tests/test_das_boundaries_gpu.py).

Recoding model: a restatement of the windowed recoding of the sort kernels and of the accumulation geometry, so that the
tests can say which reference lands where and how many references (mixed additions) a job has:
  * fold / window_digits / count_refs   msm_sort.hip: load_scalar's fold to |k| <= (r-1)/2, for_each_window_digit
  * msm_config                          msm_sort.hip: choose_msm_config (windowed recoding)
  * accumulate_lanes / seg_len          msm_accum.hip: accumulate_lanes, engine.h: accumulate_min_seg, accumulate_seg_len
  * serial_span / group_span_limit ...  msm_finalize.hip: k_bucket_finalize, k_bucket_finalize_group, launch_small_msm
"""
import bigint_twin as T
import cells_oracle as CO
import ntt_oracle as NO

R = T.R
HALF = (R - 1) // 2  # the largest folded magnitude

# ---------------------------------------------------------------- trapdoor oracle


def poly_eval(vals, x):
    acc = 0
    for c in reversed(vals):
        acc = (acc * x + c) % R
    return acc


def poly_derivative_eval(vals, x):
    acc = 0
    for i in range(len(vals) - 1, 0, -1):
        acc = (acc * x + i * vals[i]) % R
    return acc


def g1_scalar(oracle, v):
    """[v]G as the 48-byte compressed encoding"""
    return oracle.p1_compress(oracle.p1_mult(oracle.p1_generator(), v % R))


def commitment_scalar(vals, s):
    return poly_eval(vals, s)


def proof_scalar(vals, z, s, y=None):
    """Q(s) for Q = (P - y) / (X - z), y = P(z) unless given (a wrong y has no quotient: the caller must not ask)"""
    z %= R
    s %= R
    if y is None:
        y = poly_eval(vals, z)
    if s != z:
        return (poly_eval(vals, s) - y) * pow(s - z, R - 2, R) % R
    return poly_derivative_eval(vals, z)


def _div_vanishing_eval(vals, zs, s):
    """Q(s) by explicit division by X - z_i, one root after the other (used when s is one of the roots)"""
    cur = [v % R for v in vals]
    for z in zs:
        if not cur:
            break
        # synthetic division, high to low: quotient of (cur - cur(z)) by (X - z)
        q = [0] * (len(cur) - 1)
        acc = 0
        for i in range(len(cur) - 1, 0, -1):
            acc = (acc * z + cur[i]) % R
            q[i - 1] = acc
        cur = q
    return poly_eval(cur, s)


def multiproof_scalar(vals, zs, s, ys=None):
    """(P(s) - I(s)) / Z(s) for the claims ys = P(z_i) (computed when not given); the roots must be distinct"""
    zs = [z % R for z in zs]
    s %= R
    assert len(set(zs)) == len(zs)
    if s in zs:
        return _div_vanishing_eval(vals, zs, s)
    if ys is None:
        ys = [poly_eval(vals, z) for z in zs]
    zv, iv = 1, 0
    for z in zs:
        zv = zv * (s - z) % R
    for i, (zi, yi) in enumerate(zip(zs, ys)):
        num, den = 1, 1
        for j, zj in enumerate(zs):
            if j != i:
                num, den = num * (s - zj) % R, den * (zi - zj) % R
        iv = (iv + yi * num * pow(den, R - 2, R)) % R
    return (poly_eval(vals, s) - iv) * pow(zv, R - 2, R) % R


def commitment(oracle, vals, s):
    return g1_scalar(oracle, commitment_scalar(vals, s))


def proof(oracle, vals, z, s, y=None):
    return g1_scalar(oracle, proof_scalar(vals, z, s, y))


def multiproof(oracle, vals, zs, s, ys=None):
    return g1_scalar(oracle, multiproof_scalar(vals, zs, s, ys))


def secret_be(s):
    return (s % R).to_bytes(32, "big")


def cell_proof_scalars_fast(vals, K, t, s, cells=None):
    """q_j(s) for the cells of a domain of N = 2^K points, cells of l = 2^t (cells_oracle order), O(N) in all: with
    a_j = w_N^(j l) and the cell's points x_i = w_N^(j + M i),
        q_j(s) = (P(s) - I_j(s)) / (s^l - a_j),   I_j(s) = (s^l - a_j) / (l a_j) sum_i v_i x_i / (s - x_i)
    (barycentric over the coset {x : x^l = a_j}), so q_j(s) = P(s) / (s^l - a_j) - 1 / (l a_j) sum_i v_i x_i / (s - x_i).
    When s^l = a_j (s is a point of cell j) the stride-l division of cells_oracle at s.  cells: the cell ids wanted
    (all when None).  Returns {j: q_j(s)}."""
    s %= R
    N, l = 1 << K, 1 << t
    M = N >> t
    ids = range(M) if cells is None else cells
    v = CO.cells(vals, K, t)
    ps = poly_eval(vals, s)
    sl = pow(s, l, R)
    w = NO.domain_root(K)
    l_inv = pow(l, R - 2, R)
    out = {}
    for j in ids:
        a = CO.cell_root(K, t, j)
        if sl == a:
            out[j] = CO.poly_eval(CO.stride_quotient(vals, l, a), s)
            continue
        xs = [pow(w, j + M * i, R) for i in range(l)]
        inv = NO.batch_inverse([(s - x) % R for x in xs] + [(sl - a) % R, a * l % R])
        acc = sum(vi * x % R * d for vi, x, d in zip(v[j * l:(j + 1) * l], xs, inv)) % R
        out[j] = (ps * inv[l] - acc * inv[l + 1]) % R
    return out


def srs_dft_scalars(s, m):
    """the G1 DFT of the SRS (x_i = [s^i]G, i < m) over w_m: out_j = sum_i (s w^j)^i = (s^m - 1) / (s w^j - 1), and m
    where s w^j = 1"""
    s %= R
    w = NO.domain_root(NO.log2_exact(m))
    num = (pow(s, m, R) - 1) % R
    out, x = [], s
    dens = []
    for j in range(m):
        dens.append((x - 1) % R)
        x = x * w % R
    inv = NO.batch_inverse([d if d else 1 for d in dens])
    for d, di in zip(dens, inv):
        out.append(num * di % R if d else m % R)
    return out


# ---------------------------------------------------------------- torsion of E(Fp) outside G1
Z_ABS = 0xD201000000010000
H1 = (Z_ABS + 1) ** 2 // 3  # the G1 cofactor: #E(Fp) = h1 r
TORSION_ORDERS = (3, 11, 10177, 859267, 52437899)  # h1 = 3 * 11^2 * 10177^2 * 859267^2 * 52437899^2


def _curve_point(x):
    """the point of y^2 = x^3 + 4 with the smallest abscissa >= x"""
    while True:
        y2 = (x * x * x + 4) % T.P
        if pow(y2, (T.P - 1) // 2, T.P) == 1:
            return x, pow(y2, (T.P + 1) // 4, T.P)
        x += 1


def torsion_points():
    """{q: a point of order exactly q} for each prime q of the cofactor: [h1 r / q^e] R (q^e the q-part of h1) for curve
    points R until one is not infinity, then multiplied by q while that leaves it finite (E(Fp) holds all of E[q] for the
    squared primes, so [h1 r / q] R would always be infinity there)"""
    out = {}
    for q in TORSION_ORDERS:
        qe = 1
        while H1 % (qe * q) == 0:
            qe *= q
        x = 1
        while True:
            pt = T.g1_mul(_curve_point(x), H1 // qe * R)
            if pt is not T.INF:
                while T.g1_mul(pt, q) is not T.INF:
                    pt = T.g1_mul(pt, q)
                out[q] = pt
                break
            x += 1
    return out


ORDER3 = ((0, 2), (0, T.P - 2))  # x = 0: y^2 = 4


# ---------------------------------------------------------------- recoding model (msm_sort.hip)


def fold(k):
    """(|k|, negated): the representative of k mod r of magnitude at most (r-1)/2, the sign moved onto the point.
    The device centres with one signed-digit product, exact only outside r/2^31 of +-r/2 (load_scalar): there both
    representatives are valid and the digits may differ."""
    k %= R
    return (R - k, True) if k > HALF else (k, False)


def near_fold_boundary(k):
    """inside the band where the device may pick the other representative"""
    k %= R
    band = R >> 31
    return abs(k - HALF) <= band or abs(k - (R - HALF)) <= band


def window_digits(mag, c, W):
    """for_each_window_digit: signed c-bit digits, low window first, each in [-2^(c-1)+1, 2^(c-1)], the carry into the
    next window.  Returns the W digits; the top window absorbs the last carry (mag < 2^254 <= 2^(cW-1))."""
    mask, half = (1 << c) - 1, 1 << (c - 1)
    carry, out = 0, []
    for _ in range(W):
        v = (mag & mask) + carry
        mag >>= c
        neg = v > half
        out.append(v - (mask + 1) if neg else v)
        carry = 1 if neg else 0
    assert mag == 0 and carry == 0, "scalar wider than the windows"
    return out


def windows_of(c):
    return (255 + c - 1) // c


def count_refs(values, c):
    """M: the non-zero digits of all scalars (one table reference each)"""
    W = windows_of(c)
    return sum(sum(1 for d in window_digits(fold(v)[0], c, W) if d) for v in values)


def msm_config(n_srs, forced_c=None):
    """choose_msm_config, windowed recoding: (c, W, nb, max_digits) for an SRS of n_srs points"""
    best, best_c = None, 8
    for c in range(8, 21):
        if forced_c is not None and 8 <= forced_c <= 20 and c != forced_c:
            continue
        W = windows_of(c)
        if forced_c is None and 254 - c * (W - 1) < 4:  # a top window of 1-3 bits is skipped by the chooser
            continue
        cost = n_srs * W + 20.0 * (1 << (c - 1))
        if best is None or cost < best:
            best, best_c = cost, c
    W = windows_of(best_c)
    return best_c, W, 1 << (best_c - 1), W


# ---------------------------------------------------------------- accumulation / finalisation geometry

K_TINY_REFS = 65536      # engine.h kTinyRefs: jobs up to this many (bound on) references run k_small_msm
K_ACCUM_BLOCK = 256      # msm_accum.hip kAccumBlock
K_DEFAULT_LANES = 131072  # msm_accum.hip accumulate_lanes: target without KZG_ACCUM_LANES
K_SERIAL_SPAN = 16       # msm_finalize.hip kSerialSpan
K_SERIAL_SPAN_FEW = 4    # msm_finalize.hip kSerialSpanFew ...
K_FEW_BUCKETS = 2048     # ... when there are at most kFewBuckets buckets
K_CHUNK = 64             # msm_finalize.hip kChunk: pieces per tree, chunks per group
K_GROUP_SERIAL = 8       # msm_finalize.hip kGroupSerial
K_DIRECT_GROUP_REFS = 128  # msm_finalize.hip kDirectGroupRefs


def accumulate_min_seg(refs):
    # engine.h accumulate_min_seg: 4 for tiny jobs, else 8
    return 4 if refs <= K_TINY_REFS else 8


def accumulate_lanes(max_refs, target=K_DEFAULT_LANES):
    # msm_accum.hip accumulate_lanes: ceil(max_refs / min_seg(max_refs)), capped at the target (KZG_ACCUM_LANES, clamped
    # to [64, 262144]; below 64 the default), rounded up to a multiple of the workgroup
    target = K_DEFAULT_LANES if target < 64 else min(target, 262144)
    lo = accumulate_min_seg(max_refs)
    lanes = min((max_refs + lo - 1) // lo, target)
    return (lanes + K_ACCUM_BLOCK - 1) // K_ACCUM_BLOCK * K_ACCUM_BLOCK


def seg_len(M, lanes):
    # engine.h accumulate_seg_len: from the ACTUAL reference count M (lanes come from the bound max_refs)
    L = (M + lanes - 1) // lanes
    return max(L, accumulate_min_seg(M))


def serial_span(nb):
    # k_bucket_finalize: buckets of more pieces than this go to the long-bucket trees
    return K_SERIAL_SPAN_FEW if nb <= K_FEW_BUCKETS else K_SERIAL_SPAN


def finalize_group_size(nb):
    # msm_finalize.hip finalize_group_size: quads per bucket (1 = k_bucket_finalize)
    g = 1
    while g < 16 and nb * g * 2 <= 16384:
        g <<= 1
    return g


def group_span_limit(group):
    # k_bucket_finalize_group: pieces beyond which a bucket goes to the trees
    return max(K_GROUP_SERIAL * group, K_CHUNK)


def tree_span_limit(nb):
    """pieces above which the general path registers a bucket for k_heavy_tree"""
    g = finalize_group_size(nb)
    return serial_span(nb) if g == 1 else group_span_limit(g)


def small_msm(n_terms, W, small_msm_on=True):
    # api.hip enqueue_msm: max_refs = n * max_digits <= kTinyRefs -> one launch
    return small_msm_on and n_terms * W <= K_TINY_REFS


def small_msm_direct(n_terms, W, nb):
    # launch_small_msm: no accumulation phase when max_refs <= nb * 32
    return n_terms * W <= nb * 32


def pieces(s, e, L):
    """segments a bucket [s, e) touches (its 'span' in k_bucket_finalize); 1 = complete inside one segment"""
    return (e - 1) // L - s // L + 1 if e > s else 0


class Job:
    """geometry of one single-polynomial MSM of n_terms coefficients on an SRS of n_srs points"""

    def __init__(self, n_srs, n_terms, forced_c=None, lanes_target=K_DEFAULT_LANES, small_on=True):
        self.c, self.W, self.nb, self.max_digits = msm_config(n_srs, forced_c)
        self.n = n_terms
        self.max_refs = n_terms * self.max_digits
        self.lanes = accumulate_lanes(self.max_refs, lanes_target)
        self.small = small_msm(n_terms, self.W, small_on)
        self.direct = self.small and small_msm_direct(n_terms, self.W, self.nb)

    def L(self, M):
        return seg_len(M, self.lanes)


# ---------------------------------------------------------------- bucket populations from single-digit scalars
# v in 1 .. 2^(c-1) has one non-zero digit (window 0, digit v): one reference into bucket v - 1; r - v is the same
# reference with the point negated.  A list of populations therefore fixes the sorted reference list exactly: bucket b
# occupies [sum(pop[:b]), sum(pop[:b+1])), and the segments of length L cut it where the tests want.


def bucket_value(b, negate):
    return R - (b + 1) if negate else b + 1


def pieces_min_pop(k, off, L):
    """fewest references of a bucket that starts `off` references into a segment and touches exactly k segments"""
    return 1 if k == 1 else (L - off) + (k - 2) * L + 1


def pieces_max_pop(k, off, L):
    """most references of such a bucket"""
    return k * L - off


def layout(cases, L, nb, M, tail="spread", empty_run=1000):
    """Populations of nb buckets holding M references in all.  cases: (label, off, pop) in bucket order; off = the
    position inside its segment where the case bucket must start (a padding bucket in front gets it there), None = right
    after the previous bucket.  Cases that no longer fit are skipped.  The rest of the references follow after a run of
    `empty_run` empty buckets: spread over the remaining buckets ("spread") or all in the last one ("last").
    Returns (pops, placed) with placed[label] = (bucket, start, end, pieces)."""
    pops, placed = [0] * nb, {}
    cur, b = 0, 0
    reserve = 1  # the tail keeps at least one reference (the last bucket is never empty)
    for label, off, pop in cases:
        pad = 0 if off is None else (off - cur) % L
        need_b = 1 + (1 if pad else 0)
        if cur + pad + pop > M - reserve or b + need_b > nb - 1:
            continue
        if pad:
            pops[b] = pad
            b, cur = b + 1, cur + pad
        pops[b] = pop
        placed[label] = (b, cur, cur + pop, pieces(cur, cur + pop, L))
        b, cur = b + 1, cur + pop
    rest = M - cur
    first = min(b + empty_run, nb - 1)
    if tail == "last":
        pops[nb - 1] += rest
    else:
        slots = nb - first
        q, r_ = divmod(rest, slots)
        for i in range(slots):
            pops[first + i] += q + (1 if i >= slots - r_ else 0)
    assert sum(pops) == M
    return pops, placed


def values_from_pops(pops, rng, neg_fraction=0.5):
    """the single-digit scalars of a population list, in a shuffled order, a share of them negated"""
    vals = []
    for b, p in enumerate(pops):
        vals.extend(bucket_value(b, rng.random() < neg_fraction) for _ in range(p))
    rng.shuffle(vals)
    return vals


# The boundary families: cases for a job with segment length L and tree threshold S (pieces above which a bucket goes to
# k_heavy_tree).  Labels name the constant and the population that reaches it.
def family_segment_edges(L, S):
    # buckets that end one before / at / one after a segment end, cover one or two whole segments, start at the first,
    # the second or the last position of a segment (first piece from part_a or part_b)
    out = []
    for pop, what in ((L - 1, "L-1"), (L, "L"), (L + 1, "L+1"), (2 * L, "2L"), (2 * L + 1, "2L+1")):
        for off in (0, 1, L - 1):
            out.append(("seg_len pop=%s off=%d" % (what, off), off, pop))
    return out


def family_tree_threshold(L, S):
    # spans of S-1 .. S+2 pieces (S = kSerialSpan, or group_span_limit(group) when several quads share a bucket), plus
    # kSerialSpan 16/17 and kSerialSpanFew 4/5 whatever S is, each with the fewest and the most references
    out = []
    ks = [S, S + 1, S - 1, S + 2, K_SERIAL_SPAN, K_SERIAL_SPAN + 1, K_SERIAL_SPAN_FEW, K_SERIAL_SPAN_FEW + 1]
    ks = sorted(set(ks), key=ks.index)  # the job's own threshold first (small jobs have room for few cases)
    for which, fn in (("min", pieces_min_pop), ("max", pieces_max_pop)):
        for off in (0, 1, L - 1):
            for k in ks:
                out.append(("span %d pieces (S=%d) %s off=%d" % (k, S, which, off), off, fn(k, off, L)))
    return out


def family_tree_chunks(L, S):
    # kChunk = 64 pieces per tree, 64 chunks per group: spans 64k - 1, 64k, 64k + 1 and 4096 +- 1
    out = []
    for k in (63, 64, 65, 127, 128, 129, 191, 192, 193, 4095, 4096, 4097):
        out.append(("kChunk span %d min off=%d" % (k, L - 1), L - 1, pieces_min_pop(k, L - 1, L)))
        out.append(("kChunk span %d max off=0" % k, 0, pieces_max_pop(k, 0, L)))
    return out


def family_inside_segment(L, S):
    # buckets complete inside one segment at every offset, then whole-segment-only buckets back to back
    out = []
    for pop in range(1, L):
        for off in range(0, L - pop + 1):
            out.append(("inside pop=%d off=%d" % (pop, off), off, pop))
    for i in range(3):
        out.append(("whole segment %d" % i, 0 if i == 0 else None, L))
    return out


def family_staircase(L, S):
    # populations 1, 2, 3, ...: bucket boundaries fall at every offset of the segments
    return [("staircase %d" % p, 0 if p == 1 else None, p) for p in range(1, 2000)]


def family_max_heavy(L, S):
    # as many long buckets as the references allow, each S + 1 pieces of which S - 1 whole segments: the fewest owned
    # segments a registered bucket can have (the bound behind kMaxEntries / kMaxChunks1 / kMaxChunks2)
    first = ("max heavy 0 (S+1=%d pieces)" % (S + 1), L - 1, 1 + (S - 1) * L + 1)
    return [first] + [("max heavy %d" % i, None, (L - 1) + (S - 1) * L + 1) for i in range(1, 1 << 20)]


FAMILIES = {
    "segment_edges": (family_segment_edges, "spread"),
    "tree_threshold": (family_tree_threshold, "spread"),
    "tree_chunks": (family_tree_chunks, "spread"),
    "inside_segment": (family_inside_segment, "spread"),
    "staircase": (family_staircase, "spread"),
    "max_heavy": (family_max_heavy, "spread"),
    # bucket 0, a run of empty buckets up to the last one, which takes everything else
    "first_last": (lambda L, S: [("first bucket", 0, L + 1)], "last"),
}


def family_layout(name, job, M):
    """(pops, placed, L, S) of a boundary family for Job `job` with M single-digit scalars"""
    fn, tail = FAMILIES[name]
    L = job.L(M)
    S = tree_span_limit(job.nb) if not job.small else group_span_limit(finalize_group_size(job.nb))
    cases = fn(L, S)
    pops, placed = layout(cases, L, job.nb, M, tail=tail, empty_run=0 if name == "max_heavy" else 1000)
    return pops, placed, L, S


# ---------------------------------------------------------------- recoding edge scalars


def recoding_family(c):
    """scalars at the edges of the signed c-bit windows"""
    W = windows_of(c)
    half = 1 << (c - 1)
    out = [0, 1, R - 1, HALF, HALF + 1, 2, R - 2]
    # every window's digit exactly 2^(c-1) (no carry) / 2^(c-1) + 1 (a carry into every next window), below 2^254
    all_half = sum(half << (c * j) for j in range(W)) & ((1 << 254) - 1)
    all_half1 = sum((half + 1) << (c * j) for j in range(W)) & ((1 << 254) - 1)
    out += [all_half % R, all_half1 % R, R - all_half % R, R - all_half1 % R]
    # all ones up to just under the top window: the carry chain runs into the top window
    top = c * (W - 1)
    for b in (top - 1, top, top + 1, 253, 254):
        out += [((1 << b) - 1) % R, R - ((1 << b) - 1) % R]
    # every digit 1, every digit -1 (as the carry chain of 2^c - 1 values)
    out += [sum(1 << (c * j) for j in range(W) if c * j < 254) % R]
    out += [sum(((1 << c) - 1) << (c * j) for j in range(W - 1)) % R]
    # powers of two, and their negatives
    for b in range(0, 255, 7):
        out += [(1 << b) % R, R - (1 << b) % R]
    # i128-shaped values (src/scalar.rs:27-48: a <= 0 -> r - |a|)
    for a in (1, -1, (1 << 127) - 1, -(1 << 127), 12345678901234567890, -98765432109876543210):
        out.append(T.fr_from_i128(a))
    return out
