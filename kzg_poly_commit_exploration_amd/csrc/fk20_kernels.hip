// fk20_kernels.hip -- all N/l cell proofs of a batch of polynomials by FK20 (kzg_cells_and_proofs_fk20, kzg_g1_dft;
// DESIGN.md section 4.8).
//
// Domain of N = 2^K points, cells of l = 2^t, m = ceil(n / l), L the smallest power of two >= 2m.  The proof of cell j is
// q_j(s) = sum_{d <= m-2} a_j^d H_d with a_j = w_(N/l)^j and H_d = sum_i c_(i + (d+1) l) [s^i], so the proofs are the
// G1 DFT of (H_0, .., H_(m-2), 0, ..) of size N/l.  The H_d are l Toeplitz products by circulant embedding:
//     conv = IDFT_L( sum_r DFT_L(S_r) . DFT_L^Fr(R_r) ),   H_d = conv[m - 1 - d],
//     S_r[v] = [s^(v l + r)] (v < L/2, inside the SRS; infinity elsewhere),  R_r[k] = c_((m - k) l + r) (1 <= k <= m).
// (S_r may run past m: with L >= 2m those entries only ever meet zeros of R_r in the outputs that are read.)
//
// Kernels:
//   k_g1_dft_stage   one radix-2 Stockham stage of `batch` G1 DFTs (natural order in and out), one lane per butterfly.
//                    The twiddle product is a GLV ladder: w = k1 + k2 lambda with lambda = z^2 - 1 (r = lambda^2 + lambda
//                    + 1, so k1, k2 < 2^128 by one division on the host), [lambda] P = (beta x, y): 128 doublings and
//                    Shamir additions of P, phi(P), P + phi(P) instead of a 255-bit ladder.
//   k_g1_scale       [k] P for every point (the 1/m of kzg_g1_dft's inverse)
//   k_fk20_srs_gather, k_fk20_comb   the SRS side, once per (L, l): S_r from the table's level 0, and after their DFTs a
//                    comb table per base B = DFT(S_r)[i]: d 16^j B for d = 1..8, j < 64 (affine once normalised), bases in
//                    (i, r) order so that a range of positions i is a contiguous range of tables
//   k_fk20_toeplitz, k_fr_stage      R_r of every polynomial and their Fr DFTs (radix-2 Stockham, global memory); the last
//                    stage multiplies by 1/L (the G1 inverse runs unnormalised) and leaves plain integers for the digits
//   k_fk20_pointwise one lane per (polynomial, i, r) over a range of positions i: [A_r[i]] B_r[i] as 64 signed 4-bit
//                    digits, one mixed addition each from the comb table -- no doublings
//   k_fk20_fold      the sum over r: a log-depth tree, one level per launch
//   k_fk20_select    H_d = conv[m - 1 - d], zero-padded to N/l
//   k_fk20_affine_to_xyzz  kzg_g1_dft's input
//
// Bounds: the group law of g1_30.hip.h on its own outputs and on table points (section 4.2); Fr values as in
// cell_kernels.hip (canonical in and out of every stage, one product each).
#define KZG_G1_30_INLINE_DBL
#define KZG_G1_30_NO_SB
#include <hip/hip_runtime.h>

#include "engine.h"
#include "fr30.hip.h"
#include "fr30_lanes.hip.h"
#include "g1_30.hip.h"

namespace kzg {

namespace {

constexpr uint32_t kFk20Threads = 64;

// beta * 2^390 mod p, balanced radix-2^30 digits: the cube root of unity with (beta x, y) = [z^2 - 1](x, y) on G1
// (checked against the group law of oracle/bigint_twin.py)
__device__ __forceinline__ Fq fq_beta() {
    constexpr int32_t B[13] = {0x1c907181, -0x3421b7a, -0x19a8b3c1, -0xcdb8a13, 0x1c3ebc1c, -0x611979c, 0x16ffa857,
                               -0x13cb6601, 0x550bd17, 0x14cbac30, 0x17d18c86, -0x1ea6a609, 0x9c6d5};
    Fq r;
#pragma unroll
    for (int i = 0; i < kQ; i++) r.d[i] = B[i];
    return r;
}

__device__ __forceinline__ bool glv_bit(const Glv& k, int part, int bit) {
    const uint64_t w = part ? k.k2[bit >> 6] : k.k1[bit >> 6];
    return (w >> (bit & 63)) & 1;
}

// [k1 + k2 lambda] p, joint double-and-add over the 128 bits of k1 and k2
__device__ __forceinline__ XYZZ30 g1_mul_glv(const XYZZ30& p, const Glv& k) {
    XYZZ30 acc = xyzz30_inf();
    const uint64_t hi = k.k1[1] | k.k2[1], lo = k.k1[0] | k.k2[0];
    if (!(hi | lo) || xyzz30_is_inf(p)) return acc;
    const int top = hi ? 127 - __clzll(hi) : 63 - __clzll(lo);
    const Fq phix = fq_mul(p.X, fq_beta());  // phi(p) = (beta X, Y, ZZ, ZZZ)
    XYZZ30 both = p;
    {
        XYZZ30 q = p;
        q.X = phix;
        xyzz30_add(both, q);
    }
#pragma unroll 1
    for (int bit = top; bit >= 0; bit--) {
        xyzz30_dbl_body(acc);
        const uint32_t sel = (uint32_t)glv_bit(k, 0, bit) | ((uint32_t)glv_bit(k, 1, bit) << 1);
        if (sel) {
            XYZZ30 t;
#pragma unroll
            for (int i = 0; i < kQ; i++) {
                t.X.d[i] = sel == 1 ? p.X.d[i] : (sel == 2 ? phix.d[i] : both.X.d[i]);
                t.Y.d[i] = sel == 3 ? both.Y.d[i] : p.Y.d[i];
                t.ZZ.d[i] = sel == 3 ? both.ZZ.d[i] : p.ZZ.d[i];
                t.ZZZ.d[i] = sel == 3 ? both.ZZZ.d[i] : p.ZZZ.d[i];
            }
            xyzz30_add(acc, t);
        }
    }
    return acc;
}

__device__ __forceinline__ Glv load_glv(const Glv* __restrict__ t, uint32_t i) {
    const uint4* q = reinterpret_cast<const uint4*>(t + i);
    const uint4 a = q[0], b = q[1];
    Glv g;
    g.k1[0] = a.x | ((uint64_t)a.y << 32);
    g.k1[1] = a.z | ((uint64_t)a.w << 32);
    g.k2[0] = b.x | ((uint64_t)b.y << 32);
    g.k2[1] = b.z | ((uint64_t)b.w << 32);
    return g;
}

// stage s (Ns = 2^s) of `batch` DFTs of 2^log_len points: butterfly j < len/2 of vector b reads j and j + len/2, twists the
// second by w_(2 Ns)^(j mod Ns) (w^-1 for the inverse) and writes (j / Ns) 2 Ns + (j mod Ns) (+ Ns).  tw: w_(2^log_tw)^e,
// e < 2^log_tw, split.
__global__ void __launch_bounds__(kFk20Threads) k_g1_dft_stage(const uint4* __restrict__ in, uint4* __restrict__ out,
                                                               uint32_t log_len, uint32_t s, uint64_t lanes,
                                                               const Glv* __restrict__ tw, uint32_t log_tw, int inverse) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= lanes) return;
    const uint32_t half = 1u << (log_len - 1);
    const uint64_t b = t >> (log_len - 1);
    const uint32_t j = (uint32_t)t & (half - 1);
    const uint32_t k = j & ((1u << s) - 1);
    const uint4* vin = in + (b << log_len) * kXyzzU4;
    uint4* vout = out + (b << log_len) * kXyzzU4;
    XYZZ30 x = load_xyzz30(vin + (size_t)(j + half) * kXyzzU4);
    if (k) {
        const uint32_t mask = (1u << log_tw) - 1;
        uint32_t e = k << (log_tw - s - 1);
        if (inverse) e = (0u - e) & mask;
        x = g1_mul_glv(x, load_glv(tw, e));
    }
    const XYZZ30 a = load_xyzz30(vin + (size_t)j * kXyzzU4);  // after the ladder: not live across it
    const uint32_t o = ((j >> s) << (s + 1)) + k;
#pragma unroll 1
    for (int h = 0; h < 2; h++) {
        XYZZ30 r = a;
        xyzz30_add(r, x);
        store_xyzz30(vout + (size_t)(o + (h << s)) * kXyzzU4, r);
        x.Y = fq_neg(x.Y);
    }
}

__global__ void __launch_bounds__(kFk20Threads) k_g1_scale(uint4* __restrict__ io, uint64_t n, Glv k) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    store_xyzz30(io + t * kXyzzU4, g1_mul_glv(load_xyzz30(io + t * kXyzzU4), k));
}

__device__ __forceinline__ XYZZ30 xyzz30_from_record(const uint4* __restrict__ rec) {
    Affine30 p;
    p.x = load_fq16(rec);
    p.y = load_fq16(rec + 4);
    XYZZ30 a = xyzz30_inf();
    if (fq_all_zero(p.x) && fq_all_zero(p.y)) return a;
    a.X = p.x;
    a.Y = p.y;
    a.ZZ = fq_one();
    a.ZZZ = a.ZZ;
    return a;
}

// S_r[v] = SRS[v l + r] for v < L/2 inside the SRS, infinity elsewhere; out[r L + v]
__global__ void __launch_bounds__(kFk20Threads) k_fk20_srs_gather(const uint4* __restrict__ table, uint64_t srs_n,
                                                                  uint32_t log_L, uint32_t log_l, uint4* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ((uint64_t)1 << (log_L + log_l))) return;
    const uint64_t r = t >> log_L, v = t & ((1u << log_L) - 1);
    const uint64_t idx = (v << log_l) + r;
    XYZZ30 a = xyzz30_inf();
    if (v < (1u << (log_L - 1)) && idx < srs_n) a = xyzz30_from_record(table + idx * kAffineU4);
    store_xyzz30(out + t * kXyzzU4, a);
}

// bases [first, first + count) in (i, r) order, base i l + r = B[r L + i]:
// tmp[(q 64 + j) 8 + d - 1] = d 16^j B, d = 1..8, j < 64 (XYZZ)
__global__ void __launch_bounds__(kFk20Threads) k_fk20_comb(const uint4* __restrict__ B, uint32_t log_L, uint32_t log_l,
                                                            uint64_t first, uint32_t count, uint4* __restrict__ tmp) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= count) return;
    const uint64_t base_id = first + q;
    const uint64_t r = base_id & ((1u << log_l) - 1), i = base_id >> log_l;
    XYZZ30 base = load_xyzz30(B + ((r << log_L) + i) * kXyzzU4);
    uint4* o = tmp + (size_t)q * kFk20CombEntries * kXyzzU4;
#pragma unroll 1
    for (uint32_t j = 0; j < kFk20CombWindows; j++) {
        XYZZ30 run = base;
        store_xyzz30(o, run);
#pragma unroll 1
        for (uint32_t d = 2; d <= kFk20CombDigits; d++) {
            xyzz30_add(run, base);
            store_xyzz30(o + (size_t)(d - 1) * kXyzzU4, run);
        }
        o += (size_t)kFk20CombDigits * kXyzzU4;
#pragma unroll 1
        for (int i = 0; i < 4; i++) xyzz30_dbl_body(base);
    }
}

// R_r of polynomial b: out[(b l + r) L + k] = c_b[(m - k) l + r] for 1 <= k <= m inside the n uploaded coefficients, else 0
__global__ void __launch_bounds__(256) k_fk20_toeplitz(const uint32_t* __restrict__ c, uint32_t n, uint32_t m,
                                                       uint32_t log_L, uint32_t log_l, uint64_t lanes,
                                                       uint32_t* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= lanes) return;
    const uint32_t k = (uint32_t)t & ((1u << log_L) - 1);
    const uint32_t r = (uint32_t)(t >> log_L) & ((1u << log_l) - 1);
    const uint64_t b = t >> (log_L + log_l);
    uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
    if (k >= 1 && k <= m) {
        const uint64_t idx = ((uint64_t)(m - k) << log_l) + r;
        if (idx < n) {
            const uint4* src = reinterpret_cast<const uint4*>(c + 8 * (b * n + idx));
            lo = src[0];
            hi = src[1];
        }
    }
    uint4* dst = reinterpret_cast<uint4*>(out + 8 * t);
    dst[0] = lo;
    dst[1] = hi;
}

// stage s of the forward Fr DFTs of `vectors` vectors of 2^log_L values (Stockham as k_g1_dft_stage).  Values are blst_fr
// images (x 2^256), canonical; the last stage multiplies by last_c (multiplier form) and stores the plain integer.
__global__ void __launch_bounds__(256) k_fr_stage(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t log_L,
                                                  uint32_t s, uint64_t lanes, const Fr30* __restrict__ tw, int last, Fr30 last_c) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= lanes) return;
    const uint32_t half = 1u << (log_L - 1);
    const uint64_t b = t >> (log_L - 1);
    const uint32_t j = (uint32_t)t & (half - 1);
    const uint32_t k = j & ((1u << s) - 1);
    const uint32_t* vin = in + 8 * (b << log_L);
    uint32_t* vout = out + 8 * (b << log_L);
    const Fr30 a = fr30_load(vin + 8 * j);
    Fr30 x = fr30_load(vin + 8 * (j + half));
    if (k) {
        const uint32_t e22 = k << (kNttMaxLog - s - 1);  // w_(2 Ns)^k
        x = fr30_mul(x, fr30_mul(fr30_table(tw + kNttTableLen, e22 >> 11), fr30_table(tw, e22 & (kNttTableLen - 1))));
    }
    Fr30 y0 = fr30_norm(fr30_add_raw(a, x));
    Fr30 neg;
#pragma unroll
    for (int i = 0; i < kR9; i++) neg.d[i] = -x.d[i];
    Fr30 y1 = fr30_norm(fr30_add_raw(a, neg));
    if (last) {  // x 1/L, then out of the x 2^256 form: fr30_mul(v 2^256, 2^14) = v
        y0 = fr30_mul(fr30_mul(y0, last_c), fr30_small(1 << 14));
        y1 = fr30_mul(fr30_mul(y1, last_c), fr30_small(1 << 14));
    }
    const uint32_t o = ((j >> s) << (s + 1)) + k;
    fr30_store(vout + 8 * o, y0);
    fr30_store(vout + 8 * (o + (1u << s)), y1);
}

// positions [i0, i0 + ci) of every polynomial: lane (b, i', r), r fastest, i = i0 + i':
// part[lane] = [A_(b,r)[i]] B_r[i], A plain integers at scal[(b l + r) L + i], the comb table of base (i, r) at
// tab + ((i - i0) l + r) kFk20CombEntries records (a table of the chunk's bases, or of all of them with i0 = 0)
__global__ void __launch_bounds__(kFk20Threads) k_fk20_pointwise(const uint32_t* __restrict__ scal, const uint4* __restrict__ tab,
                                                                 uint32_t log_L, uint32_t log_l, uint32_t i0, uint32_t ci,
                                                                 uint64_t lanes, uint4* __restrict__ part) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= lanes) return;
    const uint32_t r = (uint32_t)t & ((1u << log_l) - 1);
    const uint64_t g = t >> log_l;  // b ci + i'
    const uint32_t ip = (uint32_t)(g % ci);
    const uint64_t b = g / ci;
    const uint32_t i = i0 + ip;
    const uint4* sp = reinterpret_cast<const uint4*>(scal + 8 * ((((b << log_l) + r) << log_L) + i));
    const uint4 s0 = sp[0], s1 = sp[1];
    const uint32_t w[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    const uint4* base = tab + ((((uint64_t)ip << log_l) + r) * kFk20CombEntries) * kAffineU4;
    XYZZ30 acc = xyzz30_inf();
    uint32_t carry = 0;
#pragma unroll 1
    for (uint32_t j = 0; j < kFk20CombWindows; j++) {
        int32_t d = (int32_t)(((w[j >> 3] >> ((j & 7) * 4)) & 15) + carry);
        carry = d > (int32_t)kFk20CombDigits;
        if (carry) d -= 16;  // scalars < 2^255: the top window is at most 7 + 1, no carry leaves it
        if (d) {
            const uint32_t mag = d < 0 ? -d : d;
            Affine30 p;
            const uint4* rec = base + (size_t)(j * kFk20CombDigits + mag - 1) * kAffineU4;
            p.x = load_fq16(rec);
            p.y = load_fq16(rec + 4);
            xyzz30_madd(acc, p, d < 0);
        }
    }
    uint4* o = log_l ? part + t * kXyzzU4 : part + ((b << log_L) + i) * kXyzzU4;  // l = 1: straight to the output
    store_xyzz30(o, acc);
}

// one level of the sum over r: part[g l + r] += part[g l + r + h] for r < h; at h = 1 group g = b ci + i' goes to
// out[b L + i0 + i']
__global__ void __launch_bounds__(kFk20Threads) k_fk20_fold(uint4* __restrict__ part, uint32_t log_l, uint32_t h, uint64_t lanes,
                                                            uint32_t log_L, uint32_t i0, uint32_t ci, uint4* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= lanes) return;
    const uint64_t g = t / h, r = t % h;
    uint4* at = part + ((g << log_l) + r) * kXyzzU4;
    XYZZ30 a = load_xyzz30(at);
    xyzz30_add(a, load_xyzz30(at + (size_t)h * kXyzzU4));
    store_xyzz30(h == 1 ? out + (((g / ci) << log_L) + i0 + g % ci) * kXyzzU4 : at, a);
}

// H[b M + d] = conv[b L + m - 1 - d] for d <= m - 2, infinity up to M
__global__ void __launch_bounds__(256) k_fk20_select(const uint4* __restrict__ conv, uint32_t log_L, uint32_t m, uint32_t log_M,
                                                     uint64_t lanes, uint4* __restrict__ H) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= lanes) return;
    const uint64_t b = t >> log_M;
    const uint32_t d = (uint32_t)t & ((1u << log_M) - 1);
    uint4* o = H + t * kXyzzU4;
    if (d + 2 <= m) {
        const uint4* src = conv + ((b << log_L) + (m - 1 - d)) * kXyzzU4;
#pragma unroll
        for (int q = 0; q < (int)kXyzzU4; q++) o[q] = src[q];
    } else {
        const uint4 zero = make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < (int)kXyzzU4; q++) o[q] = zero;
    }
}

__global__ void __launch_bounds__(256) k_fk20_affine_to_xyzz(const uint4* __restrict__ aff, uint64_t n, uint4* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    store_xyzz30(out + t * kXyzzU4, xyzz30_from_record(aff + t * kAffineU4));
}

dim3 grid_for(uint64_t lanes, uint32_t threads) { return dim3((unsigned)((lanes + threads - 1) / threads)); }

}  // namespace

const void* launch_g1_dft(hipStream_t s, const void* d_in, void* d_a, void* d_b, uint32_t log_len, uint64_t batch,
                          const Glv* d_tw, uint32_t log_tw, bool inverse) {
    const void* cur = d_in;
    const uint64_t lanes = batch << (log_len ? log_len - 1 : 0);
    for (uint32_t st = 0; st < log_len; st++) {
        void* dst = (st & 1) ? d_b : d_a;
        hipLaunchKernelGGL(k_g1_dft_stage, grid_for(lanes, kFk20Threads), dim3(kFk20Threads), 0, s, (const uint4*)cur,
                           (uint4*)dst, log_len, st, lanes, d_tw, log_tw, inverse ? 1 : 0);
        cur = dst;
    }
    return cur;
}

void launch_g1_scale(hipStream_t s, void* d_io, uint64_t n, const Glv& k) {
    if (!n) return;
    hipLaunchKernelGGL(k_g1_scale, grid_for(n, kFk20Threads), dim3(kFk20Threads), 0, s, (uint4*)d_io, n, k);
}

void launch_fk20_srs_gather(hipStream_t s, const void* d_table, uint64_t srs_n, uint32_t log_L, uint32_t log_l, void* d_out) {
    const uint64_t lanes = (uint64_t)1 << (log_L + log_l);
    hipLaunchKernelGGL(k_fk20_srs_gather, grid_for(lanes, kFk20Threads), dim3(kFk20Threads), 0, s, (const uint4*)d_table, srs_n,
                       log_L, log_l, (uint4*)d_out);
}

void launch_fk20_comb(hipStream_t s, const void* d_bases, uint32_t log_L, uint32_t log_l, uint64_t first, uint32_t count,
                      void* d_tmp) {
    if (!count) return;
    hipLaunchKernelGGL(k_fk20_comb, grid_for(count, kFk20Threads), dim3(kFk20Threads), 0, s, (const uint4*)d_bases, log_L, log_l,
                       first, count, (uint4*)d_tmp);
}

const uint32_t* launch_fk20_fr_side(hipStream_t s, const uint32_t* d_coeffs, uint32_t n, uint32_t m, uint32_t log_L,
                                    uint32_t log_l, uint64_t batch, const void* d_tw, const Fr30& inv_L, uint32_t* d_a,
                                    uint32_t* d_b) {
    const uint64_t vals = batch << (log_L + log_l);
    hipLaunchKernelGGL(k_fk20_toeplitz, grid_for(vals, 256), dim3(256), 0, s, d_coeffs, n, m, log_L, log_l, vals, d_a);
    const uint64_t lanes = vals >> 1;
    uint32_t* cur = d_a;
    for (uint32_t st = 0; st < log_L; st++) {
        uint32_t* dst = (st & 1) ? d_a : d_b;
        hipLaunchKernelGGL(k_fr_stage, grid_for(lanes, 256), dim3(256), 0, s, (const uint32_t*)cur, dst, log_L, st, lanes,
                           (const Fr30*)d_tw, st + 1 == log_L ? 1 : 0, inv_L);
        cur = dst;
    }
    return cur;
}

const uint32_t* launch_fr_dft(hipStream_t s, const uint32_t* d_in, uint32_t* d_a, uint32_t* d_b, uint32_t log_len, uint64_t batch,
                              const void* d_tw) {
    const uint64_t lanes = batch << (log_len ? log_len - 1 : 0);
    const uint32_t* cur = d_in;
    for (uint32_t st = 0; st < log_len; st++) {
        uint32_t* dst = cur == d_a ? d_b : d_a;
        hipLaunchKernelGGL(k_fr_stage, grid_for(lanes, 256), dim3(256), 0, s, cur, dst, log_len, st, lanes, (const Fr30*)d_tw, 0,
                           fr30_zero());
        cur = dst;
    }
    return cur;
}

void launch_fk20_pointwise(hipStream_t s, const uint32_t* d_scal, const void* d_tab, uint32_t log_L, uint32_t log_l,
                           uint32_t i0, uint32_t ci, uint64_t batch, void* d_part, void* d_out) {
    const uint64_t lanes = (batch * ci) << log_l;
    hipLaunchKernelGGL(k_fk20_pointwise, grid_for(lanes, kFk20Threads), dim3(kFk20Threads), 0, s, d_scal, (const uint4*)d_tab,
                       log_L, log_l, i0, ci, lanes, (uint4*)(log_l ? d_part : d_out));
    const uint64_t groups = batch * ci;
    for (uint32_t h = (1u << log_l) >> 1; h >= 1; h >>= 1)
        hipLaunchKernelGGL(k_fk20_fold, grid_for(groups * h, kFk20Threads), dim3(kFk20Threads), 0, s, (uint4*)d_part, log_l, h,
                           groups * h, log_L, i0, ci, (uint4*)d_out);
}

void launch_fk20_select(hipStream_t s, const void* d_conv, uint32_t log_L, uint32_t m, uint32_t log_M, uint64_t batch, void* d_H) {
    const uint64_t lanes = batch << log_M;
    hipLaunchKernelGGL(k_fk20_select, grid_for(lanes, 256), dim3(256), 0, s, (const uint4*)d_conv, log_L, m, log_M, lanes,
                       (uint4*)d_H);
}

void launch_affine_to_xyzz(hipStream_t s, const void* d_affine, uint64_t n, void* d_out) {
    if (!n) return;
    hipLaunchKernelGGL(k_fk20_affine_to_xyzz, grid_for(n, 256), dim3(256), 0, s, (const uint4*)d_affine, n, (uint4*)d_out);
}

}  // namespace kzg
