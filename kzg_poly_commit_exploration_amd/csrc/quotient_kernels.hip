// quotient_kernels.hip -- the quotient of a permutation argument on a coset (kzg_coset_extend, kzg_permutation_constraints_coset,
// kzg_vanishing_quotient, kzg_permutation_quotient).
//
// n = 2^k, H = <w_n>, N = rot n (rot = 2^x, x <= 3), coset points x_i = g w_N^i (g = 7, natural order, i < N).  With t wire
// columns f_j, t permutation columns s_j, the accumulator z, the shifts k_j and the challenges alpha, beta, gamma, all given by
// their N values on the coset:
//
//     Num(x_i) = G_i + alpha  [ z_i prod_j (f_j[i] + beta k_j x_i + gamma)  -  z_(i + rot) prod_j (f_j[i] + beta s_j[i] + gamma) ]
//                    + alpha^2 (z_i - 1) L0_i
//     out_i    = Num(x_i) / Z_H(x_i),        Z_H(x_i) = g^n w_rot^(i mod rot) - 1:   rot values, inverted by the host
//
// z(w X) on the coset is z at index (i + rot) mod N; L0_i are the values of L_0(X) = (X^n - 1) / (n (X - 1)) = (1/n) sum_(k<n) X^k,
// one more extended column; G is the caller's gate term (null: 0).
//
// Kernels:
//   k_pq_constraints  one coset point per lane, kPqTile = 256 lanes per workgroup.  The columns are walked one after another with
//                     the two running products A (from z_i) and B (from z_(i + rot)): the register state does not grow with t.
//                     x_i is never formed: beta k_j g arrives prepared and w_N^i comes from the forward NTT twiddles (lo x hi).
//                     The division by Z_H is the last product, with the stored multiplier zinv[i mod rot].
//   k_pq_pad_twist    out[b N + i] = in[b stride + i] g^i c for i < len, 0 for len <= i < N (in = null: every in-value is `fill`).
// The transforms, the division of a caller's own numerator and the untwist with its flag are ntt_kernels.hip's,
// fk20_kernels.hip's and recover_kernels.hip's.
//
// Forms (fr30.hip.h; fr30_mul(a, b) = a b / 2^270).  An IMAGE is x 2^256 (what the ABI holds), a MULTIPLIER x 2^270.
// image x multiplier = image, multiplier x multiplier = multiplier, image x image = x y 2^242: neither.
//   f_j[i], s_j[i], z_i, L0_i, G_i, gamma, one, (beta k_j g)   images (loaded canonical, or prepared by the host).
//   w_N^i, beta, zinv[.], g^i, c                               multipliers (tables, or prepared by the host).
//   a_j = f_j + gamma + (beta k_j g) w_N^i,  b_j = f_j + gamma + s_j beta        sums of images: images.
//   A = z_i a_0 .. a_(t-1), B = z_(i+rot) b_0 .. b_(t-1)       t + 1 images by t products: X 2^(256 - 14 t).
//   D = A - B                                                  the same form; alpha1 = alpha 2^(270 + 14 t) (a "multiplier" that
//                                                              also carries 2^(14 t)) takes it to the IMAGE of alpha (A' - B').
//   (z_i - one) L0_i                                           image x image = X 2^242; alpha2 = alpha^2 2^(270 + 14) makes it
//                                                              the IMAGE of alpha^2 (z_i - 1) L0_i.
//   S = G_i + alpha1 D + alpha2 (..)                           a sum of images; out_i = S x zinv: image, stored canonical.
//
// Bounds.  A loaded value is canonical, [0, r), in carry-normalised digits (fr30_from_limbs).  A product returns
// |v| <= 0.5001 r + |a b| / 2^270 with digits 0..7 in [-2^29, 2^29).
//   f_j + gamma                one carry pass over two normalised values (raw digits within 2^30 + 8), [0, 2 r).
//   a_j, b_j                   that plus one product (raw digits below 2^30 + 4, inside what fr30_norm takes):
//                              (-0.51 r, 2.51 r), normalised digits, top digit below 2.51 x 0x73ee.  Operands of products ONLY.
//   A, B                       first operand z canonical (< r), then products: |A a_j| / 2^270 <= 2.51 r^2 / 2^270 < r / 2^13, so
//                              |A|, |B| <= 0.5002 r after every step.
//   D = A - B                  digit-wise difference of two products (|digit| < 2^30), one carry pass: |D| <= 1.0004 r.  An
//                              operand of the product with alpha1 only.
//   z_i - one                  difference of two canonical values (raw digits within 2^30 + 8), one carry pass: (-r, r).  An
//                              operand only.
//   S                          canonical G_i (or nothing) plus two products, each added with its own carry pass (one product per
//                              pass, as fr30_mac: raw digits within 2^30 + 4): (-1.0004 r, 2.0004 r), top digit below
//                              2.01 x 0x73ee.  It is NOT inside what fr30_to_limbs canonicalises and is never stored or tested: it
//                              is the operand of the product with zinv (canonical multiplier), whose result,
//                              |v| <= 0.5001 r + 2.01 r^2 / 2^270, is stored through fr30_to_limbs.  So the sum is folded by the
//                              product that follows it and needs no fr30_sum_reduce.
// No zero test is made in k_pq_constraints at all (whether Num is divisible shows in the untwist's flag, which tests canonical
// residues).  k_pq_pad_twist: value x (g^i c), two products, stored canonical.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "fr30.hip.h"
#include "fr30_lanes.hip.h"

namespace kzg {

namespace {

static_assert(kPqTile == 256, "one coset point per lane of a 256-lane workgroup");

struct PqArgs {
    const uint32_t* wires;   // t columns of N values, column j at + 8 j stride words
    const uint32_t* sigmas;
    const uint32_t* z;       // N values
    const uint32_t* l0;      // N values
    const uint32_t* gate;    // N values or null
    const uint32_t* zinv;    // rot stored multipliers: 1 / Z_H(x_i) by i mod rot
    const Fr30* tw;          // the forward NTT twiddles
    uint32_t log_N, rot, t;
    size_t stride;
    Fr30 beta;               // multiplier
    Fr30 gamma, one;         // images
    Fr30 alpha1, alpha2;     // alpha 2^(270 + 14 t), alpha^2 2^(270 + 14)
    Fr30 bkg[kPqMaxColumns]; // beta k_j g, images
};

__global__ void __launch_bounds__(kPqTile) k_pq_constraints(PqArgs in, uint32_t* __restrict__ out) {
    const uint32_t N = 1u << in.log_N;
    const uint32_t i = blockIdx.x * kPqTile + threadIdx.x;
    if (i >= N) return;
    const uint32_t ir = (i + in.rot) & (N - 1);
    const Fr30 zi = fr30_load(in.z + 8 * (size_t)i);
    // S = G_i + alpha^2 (z_i - 1) L0_i
    Fr30 sum = fr30_mul(fr30_mul(fr30_sub(zi, in.one), fr30_load(in.l0 + 8 * (size_t)i)), in.alpha2);
    if (in.gate) sum = fr30_add(fr30_load(in.gate + 8 * (size_t)i), sum);
    // the two running products over the columns
    Fr30 a = zi, b = fr30_load(in.z + 8 * (size_t)ir);
    const Fr30 w = fr30_root(in.tw, i, in.log_N);
    const uint32_t* pf = in.wires + 8 * (size_t)i;
    const uint32_t* ps = in.sigmas + 8 * (size_t)i;
#pragma unroll 1
    for (uint32_t j = 0; j < in.t; j++) {
        const Fr30 fg = fr30_add(fr30_load(pf), in.gamma);                 // [0, 2 r)
        a = fr30_mul(a, fr30_add(fg, fr30_mul(in.bkg[j], w)));           // the factor (-0.51 r, 2.51 r): an operand only
        b = fr30_mul(b, fr30_add(fg, fr30_mul(fr30_load(ps), in.beta)));
        pf += 8 * in.stride;
        ps += 8 * in.stride;
    }
    sum = fr30_add(sum, fr30_mul(fr30_sub(a, b), in.alpha1));              // (-1.0004 r, 2.0004 r): an operand only
    fr30_store(out + 8 * (size_t)i, fr30_mul(sum, fr30_load(in.zinv + 8 * (size_t)(i & (in.rot - 1)))));
}

// lane (b, i): out[b N + i] = in[b stride + i] g^i c (i < len), 0 (len <= i < N)
__global__ void __launch_bounds__(kPqTile) k_pq_pad_twist(const uint32_t* __restrict__ in, size_t stride, uint32_t len, Fr30 fill,
                                                          uint32_t log_N, uint64_t lanes, const Fr30* __restrict__ gtab, Fr30 c,
                                                          uint32_t* __restrict__ out) {
    const uint64_t lane = (uint64_t)blockIdx.x * kPqTile + threadIdx.x;
    if (lane >= lanes) return;
    const uint32_t i = (uint32_t)lane & ((1u << log_N) - 1);
    const uint64_t b = lane >> log_N;
    if (i >= len) {
        uint4* q = reinterpret_cast<uint4*>(out + 8 * lane);
        q[0] = q[1] = make_uint4(0, 0, 0, 0);
        return;
    }
    const Fr30 v = in ? fr30_load(in + 8 * (b * stride + i)) : fill;
    fr30_store(out + 8 * lane, fr30_mul(v, fr30_mul(fr30_pow22(gtab, i), c)));
}

}  // namespace

void launch_pq_constraints(hipStream_t s, const PqColumns& cols, uint32_t log_N, uint32_t rot, uint32_t t, size_t stride,
                           const PqScalars& sc, const void* d_tw, uint32_t* d_out) {
    PqArgs in{};
    in.wires = cols.d_wires;
    in.sigmas = cols.d_sigmas;
    in.z = cols.d_z;
    in.l0 = cols.d_l0;
    in.gate = cols.d_gate;
    in.zinv = cols.d_zinv;
    in.tw = (const Fr30*)d_tw;
    in.log_N = log_N;
    in.rot = rot;
    in.t = t;
    in.stride = stride;
    in.beta = *sc.beta;
    in.gamma = *sc.gamma;
    in.one = *sc.one;
    in.alpha1 = *sc.alpha1;
    in.alpha2 = *sc.alpha2;
    for (uint32_t j = 0; j < t && j < kPqMaxColumns; j++) in.bkg[j] = sc.bkg[j];
    const uint32_t N = 1u << log_N;
    hipLaunchKernelGGL(k_pq_constraints, dim3((N + kPqTile - 1) / kPqTile), dim3(kPqTile), 0, s, in, d_out);
}

void launch_pq_pad_twist(hipStream_t s, const uint32_t* d_in, size_t stride, uint32_t len, const Fr30& fill, uint32_t log_N,
                         uint64_t batch, const void* d_gtab, const Fr30& c, uint32_t* d_out) {
    const uint64_t lanes = batch << log_N;
    hipLaunchKernelGGL(k_pq_pad_twist, dim3((unsigned)((lanes + kPqTile - 1) / kPqTile)), dim3(kPqTile), 0, s, d_in, stride, len, fill,
                       log_N, lanes, (const Fr30*)d_gtab, c, d_out);
}

}  // namespace kzg
