// circuit_kernels.hip -- the quotient of a circuit whose key is resident: the arithmetic gate evaluated in the same walk over the
// columns as the permutation constraints (kzg_circuit_quotient).
//
// Domain, coset and notation are quotient_kernels.hip's: n = 2^k, N = rot n, x_i = g w_N^i (g = 7, natural order).  With t wire
// columns f_j, the resident selectors q_j (j < t), q_M, q_C and permutation columns s_j, the accumulator z, the public inputs PI
// and the caller's term G', all given by their N values on the coset:
//
//     Gate(x_i) = sum_j q_j[i] f_j[i] + q_M[i] f_0[i] f_1[i] + q_C[i] + PI_i + G'_i
//     Num(x_i)  = Gate(x_i) + alpha [ z_i prod_j (f_j[i] + beta k_j x_i + gamma) - z_(i + rot) prod_j (f_j[i] + beta s_j[i] + gamma) ]
//                           + alpha^2 (z_i - 1) L0_i
//     out_i     = Num(x_i) / Z_H(x_i)
//
// Kernel:
//   k_ck_constraints  k_pq_constraints with the gate accumulated beside the two running products: one coset point per lane,
//                     kPqTile = 256 lanes per workgroup, the column loop not unrolled.  A column costs one more load (q_j[i]) and
//                     one more product (q_j f_j) on the wire value that is in registers anyway; f_0 stays in registers until the
//                     q_M term closes at j = 1 (two products and one scaling).  Nothing intermediate is stored.
//
// Forms (fr30.hip.h; fr30_mul(a, b) = a b / 2^270; IMAGE = x 2^256, MULTIPLIER = x 2^270).  EVERY resident column is stored as
// images (what kzg_coset_extend writes and kzg_circuit_column_device hands out), the selectors included: the gate's products are
// therefore image x image and the kernel pays the scaling itself, once per point and not once per column:
//   q_j[i] f_j[i]                                  image x image = X 2^242.
//   m = (f_0 f_1) k14                              f_0 f_1 is X 2^242; k14 = 2^(270 + 14) (2^14 in multiplier form) makes it
//                                                  the IMAGE of f_0 f_1.
//   q_M[i] m                                       image x image = X 2^242, the form of the linear terms.
//   P = sum_j q_j f_j + q_M m                      a sum of t + 1 values of the form X 2^242.
//   P k14                                          the IMAGE of sum_j q_j f_j + q_M f_0 f_1.
//   q_C[i], PI_i, G'_i                             images, loaded canonical.
//   the permutation part and alpha^2 (z_i - 1) L0_i   as in quotient_kernels.hip (alpha1 = alpha 2^(270 + 14 t),
//                                                  alpha2 = alpha^2 2^(270 + 14)): images.
//   S = q_C + PI + G' + P k14 + alpha2 (..) + alpha1 D   a sum of images; out_i = S x zinv: image, stored canonical.
//
// Bounds.  A loaded value is canonical, [0, r), in carry-normalised digits.  A product returns |v| <= 0.5001 r + |a b| / 2^270
// with digits 0..7 in [-2^29, 2^29); r^2 / 2^270 < r / 2^15.
//   q_j f_j, f_0 f_1, q_M m    canonical x canonical (m: |m| <= 0.5002 r): |v| <= 0.5001 r + r^2 / 2^270 < 0.5002 r.
//   P                          zero, then t + 1 <= 8 such products, each added with its own carry pass (one product per pass, as
//                              fr30_mac: raw digits within 2^30 + 4): |P| <= 8 x 0.5002 r < 4.002 r, normalised digits 0..7, top
//                              digit below 4.002 x 0x73ee + 1 < 2^17.  An operand of the product with k14 ONLY.
//   P k14                      k14 canonical (< r): |v| <= 0.5001 r + 4.002 r^2 / 2^270 < 0.5003 r.
//   S                          starts as the product alpha2 (..) (|v| <= 0.5003 r, as in quotient_kernels.hip), then up to three
//                              canonical values (q_C always, PI and G' when given), then the two products P k14 and alpha1 D; every
//                              addition has its own carry pass and adds either one product (raw digits within 2^30 + 4) or one
//                              normalised canonical value (2^30 + 8), inside what fr30_norm takes.
//                              S in (-1.501 r, 4.501 r): normalised digits 0..7, top digit below 4.501 x 0x73ee + 1 < 2^18.
//                              Not inside what fr30_to_limbs canonicalises and never stored or tested: it is the operand of the
//                              last product, with zinv (canonical multiplier): |S zinv| / 2^270 <= 4.501 r^2 / 2^270 < r / 2^12.
//                              A column of that product is at most 9 x (2^29 + 4)^2 + 3.7 x 2^58 < 2^62 (the top digit is far
//                              below 2^29 + 4), so the sum stays inside what fr30_mul takes and needs NO fr30_sum_reduce; the
//                              result, |v| <= 0.5004 r, is stored through fr30_to_limbs, which takes (-r, 2 r).
//   a_j, b_j, A, B, D          as in quotient_kernels.hip.
// No zero test is made (whether Num is divisible shows in the untwist's flag, which tests canonical residues).
#include <hip/hip_runtime.h>

#include "engine.h"
#include "fr30.hip.h"
#include "fr30_lanes.hip.h"

namespace kzg {

namespace {

static_assert(kPqTile == 256, "one coset point per lane of a 256-lane workgroup");

struct CkArgs {
    const uint32_t* wires;   // t columns of N values, column j at + 8 j stride words (the call's workspace)
    const uint32_t* q_lin;   // t resident columns of N values, column j at + 8 j N words
    const uint32_t* sigmas;  // the same
    const uint32_t* q_mul;   // N values each
    const uint32_t* q_const;
    const uint32_t* z;
    const uint32_t* l0;
    const uint32_t* pi;      // N values or null
    const uint32_t* gate;    // N values or null
    const uint32_t* zinv;    // rot stored multipliers: 1 / Z_H(x_i) by i mod rot
    const Fr30* tw;          // the forward NTT twiddles
    uint32_t log_N, rot, t;
    size_t stride;
    Fr30 beta;               // multiplier
    Fr30 gamma, one;         // images
    Fr30 alpha1, alpha2;     // alpha 2^(270 + 14 t), alpha^2 2^(270 + 14)
    Fr30 k14;                // 2^(270 + 14)
    Fr30 bkg[kPqMaxColumns]; // beta k_j g, images
};

__global__ void __launch_bounds__(kPqTile) k_ck_constraints(CkArgs in, uint32_t* __restrict__ out) {
    const uint32_t N = 1u << in.log_N;
    const uint32_t i = blockIdx.x * kPqTile + threadIdx.x;
    if (i >= N) return;
    const uint32_t ir = (i + in.rot) & (N - 1);
    const Fr30 zi = fr30_load(in.z + 8 * (size_t)i);
    // S = q_C + PI + G' + alpha^2 (z_i - 1) L0_i
    Fr30 sum = fr30_mul(fr30_mul(fr30_sub(zi, in.one), fr30_load(in.l0 + 8 * (size_t)i)), in.alpha2);
    sum = fr30_add(fr30_load(in.q_const + 8 * (size_t)i), sum);
    if (in.pi) sum = fr30_add(fr30_load(in.pi + 8 * (size_t)i), sum);
    if (in.gate) sum = fr30_add(fr30_load(in.gate + 8 * (size_t)i), sum);
    // the two running products and the gate's products over the columns
    Fr30 a = zi, b = fr30_load(in.z + 8 * (size_t)ir);
    Fr30 p = fr30_zero(), f0 = fr30_zero();
    const Fr30 w = fr30_root(in.tw, i, in.log_N);
    const uint32_t* pf = in.wires + 8 * (size_t)i;
    const uint32_t* pq = in.q_lin + 8 * (size_t)i;
    const uint32_t* ps = in.sigmas + 8 * (size_t)i;
#pragma unroll 1
    for (uint32_t j = 0; j < in.t; j++) {
        const Fr30 f = fr30_load(pf);
        p = fr30_mac(p, fr30_load(pq), f);                                 // q_j f_j: X 2^242
        if (j == 0) f0 = f;
        if (j == 1) p = fr30_mac(p, fr30_mul(fr30_mul(f0, f), in.k14), fr30_load(in.q_mul + 8 * (size_t)i));  // q_M f_0 f_1
        const Fr30 fg = fr30_add(f, in.gamma);                           // [0, 2 r)
        a = fr30_mul(a, fr30_add(fg, fr30_mul(in.bkg[j], w)));           // the factor (-0.51 r, 2.51 r): an operand only
        b = fr30_mul(b, fr30_add(fg, fr30_mul(fr30_load(ps), in.beta)));
        pf += 8 * in.stride;
        pq += 8 * (size_t)N;
        ps += 8 * (size_t)N;
    }
    sum = fr30_add(sum, fr30_mul(p, in.k14));                            // |p| < 4.002 r: an operand only
    sum = fr30_add(sum, fr30_mul(fr30_sub(a, b), in.alpha1));              // (-1.501 r, 4.501 r): an operand only
    fr30_store(out + 8 * (size_t)i, fr30_mul(sum, fr30_load(in.zinv + 8 * (size_t)(i & (in.rot - 1)))));
}

}  // namespace

void launch_ck_constraints(hipStream_t s, const CkColumns& cols, uint32_t log_N, uint32_t rot, uint32_t t, size_t stride,
                           const PqScalars& sc, const Fr30& k14, const void* d_tw, uint32_t* d_out) {
    CkArgs in{};
    in.wires = cols.d_wires;
    in.q_lin = cols.d_q_lin;
    in.sigmas = cols.d_sigmas;
    in.q_mul = cols.d_q_mul;
    in.q_const = cols.d_q_const;
    in.z = cols.d_z;
    in.l0 = cols.d_l0;
    in.pi = cols.d_pi;
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
    in.k14 = k14;
    for (uint32_t j = 0; j < t && j < kPqMaxColumns; j++) in.bkg[j] = sc.bkg[j];
    const uint32_t N = 1u << log_N;
    hipLaunchKernelGGL(k_ck_constraints, dim3((N + kPqTile - 1) / kPqTile), dim3(kPqTile), 0, s, in, d_out);
}

}  // namespace kzg
