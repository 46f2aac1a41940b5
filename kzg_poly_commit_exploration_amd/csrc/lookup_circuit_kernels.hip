// lookup_circuit_kernels.hip -- the lookup argument (LogUp) of a circuit whose key holds a table: the folded columns the
// multiplicities and the running sum are made from, and the lookup's term of the quotient's numerator on the coset
// (kzg_circuit_lookup_columns, kzg_circuit_lookup_quotient).
//
// Domain, coset and notation are circuit_kernels.hip's: n = 2^k, N = rot n, x_i = g w_N^i.  A lookup circuit keeps c <= t table
// columns tab_j and one selector q_K beside the key of section 4.22.  With the challenges theta, beta and alpha, the first c wire
// columns f_j, the multiplicities m and the running sum phi:
//
//     f[i]  = q_K[i] sum_{j<c} theta^j f_j[i]            T[i] = sum_{j<c} theta^j tab_j[i]            (over H: k_lk_fold)
//     F     = beta + q_K sum_j theta^j f_j               Tt   = beta + sum_j theta^j tab_j            (on the coset)
//     Lk1   = (phi(w X) - phi(X)) F Tt - Tt + m F        Lk2  = L_0 phi
//     G'    = alpha^3 Lk1 + alpha^4 Lk2                                                               (k_lk_constraints)
//
// Kernels (one element per lane, kPqTile = 256 lanes per workgroup, the column loops not unrolled, nothing intermediate stored):
//   k_lk_fold         n lanes: row i of the c wires (at a stride), of the c resident table columns and of q_K -> f[i], T[i].
//                     What kzg_lookup_multiplicities' and kzg_lookup_sum's kernels read as their one lookup column and their
//                     table; those add beta themselves.
//   k_lk_constraints  N lanes: point i of the extended wires, of the resident coset forms of tab_j, q_K and L_0 and of the
//                     extensions of m and phi (phi also at i + rot mod N, the point w x_i, as z is read in k_ck_constraints)
//                     -> G'_i, written where k_ck_constraints reads its caller's term.
//
// Forms (fr30.hip.h; fr30_mul(a, b) = a b / 2^270; IMAGE = x 2^256, MULTIPLIER = x 2^270).  Every column is stored as images.
//   th_j                       theta^j in multiplier form (th_0 = 2^270): image x multiplier = image.
//   s_f = sum_j f_j th_j       a sum of c images; s_t = sum_j tab_j th_j the same.
//   (s_f q_K) k14              image x image = X 2^242; k14 = 2^(270 + 14) makes it the IMAGE of q_K sum_j theta^j f_j.
//   k_lk_fold: f = that product, T = s_t x one (2^270: the value unchanged, the magnitude reduced).
//   F = beta + (s_f q_K) k14,  Tt = beta + s_t                 beta as the digits of its image: images.
//   D = phi_(i + rot) - phi_i                                  image.
//   E = (D Tt) k14 + m_i                                       D Tt is X 2^242, k14 makes it an image; m_i an image.
//   Q = (E F) k14                                              the IMAGE of F ((phi(w X) - phi(X)) Tt + m).
//   V = (L0_i phi_i) ak14                                      ak14 = alpha 2^(270 + 14): the IMAGE of alpha L_0 phi.
//   W = Q - Tt + V                                             the image of Lk1 + alpha Lk2.
//   G'_i = W a3                                                a3 = alpha^3 in multiplier form: image, stored canonical.
//
// Bounds.  A loaded value is canonical, [0, r), in carry-normalised digits.  A product returns |v| <= 0.5001 r + |a b| / 2^270
// with digits 0..7 in [-2^29, 2^29); r^2 / 2^270 < r / 2^15.
//   s_f, s_t      zero, then c <= 7 products canonical x canonical multiplier (each |v| < 0.5002 r), each added with its own carry
//                 pass (fr30_mac: one product per pass, raw digits within 2^30 + 4): |s| < 7 x 0.5002 r < 3.502 r, normalised
//                 digits 0..7, top digit below 3.502 x 0x73ee + 1 < 2^17.  Operands of a product or of one addition only.
//   s_f q_K       |v| <= 0.5001 r + 3.502 r^2 / 2^270 < 0.5003 r; times k14 (canonical): < 0.5002 r.  k_lk_fold stores it
//                 through fr30_to_limbs, which takes (-r, 2 r).
//   s_t x one     |one270| < r / 2: |v| <= 0.5001 r + 3.502 r (r / 2) / 2^270 < 0.5002 r, stored through fr30_to_limbs.
//   F             canonical beta plus one product: (-0.5002 r, 1.5002 r), one carry pass (raw digits within 2^30 + 8).
//   Tt            canonical beta plus s_t: (-3.502 r, 4.502 r), one carry pass, top digit below 2^18.  An operand of one product and
//                 of one subtraction only.
//   D             canonical minus canonical: (-r, r), one carry pass.
//   D Tt          |v| <= 0.5001 r + 4.502 r^2 / 2^270 < 0.5003 r; times k14: < 0.5002 r.
//   E             one product plus canonical m_i: (-0.5002 r, 1.5002 r), one carry pass.
//   E F           |v| <= 0.5001 r + 1.5002^2 r^2 / 2^270 < 0.5002 r; times k14: Q, < 0.5002 r.
//   L0 phi, V     canonical x canonical, then times ak14 (canonical): < 0.5002 r.
//   W             Q - Tt (one carry pass: raw digits within 2^30 + 8), then + V (one more): |W| < 0.5002 r + 4.502 r + 0.5002 r
//                 < 5.503 r, normalised digits 0..7, top digit below 5.503 x 0x73ee + 1 < 2^18.  Never stored or tested: it is the
//                 operand of the last product, with a3 (canonical): a column of that product is at most 9 x (2^29 + 4)^2 +
//                 3.7 x 2^58 < 2^62, inside what fr30_mul takes.
//   G'_i          |v| <= 0.5001 r + 5.503 r^2 / 2^270 < 0.5003 r, stored through fr30_to_limbs.
// No zero test is made: a tuple outside the table shows in the multiplicities' flag, a zero denominator in the running sum's, a
// false phi or m in the quotient's remainder.
// Indices: i < N <= 2^22; every column offset (8 j stride + 8 i words) is formed in 64 bits.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "fr30.hip.h"
#include "fr30_lanes.hip.h"

namespace kzg {

namespace {

static_assert(kPqTile == 256, "one row or coset point per lane of a 256-lane workgroup");

// sum_{j < c} col_j th_j: column j at p + 8 j stride words
__device__ __forceinline__ Fr30 lk_folded(const uint32_t* __restrict__ p, size_t stride, uint32_t c, const Fr30* th) {
    Fr30 s = fr30_zero();
#pragma unroll 1
    for (uint32_t j = 0; j < c; j++) {
        s = fr30_mac(s, fr30_load(p), th[j]);
        p += 8 * stride;
    }
    return s;
}

struct LkFoldArgs {
    const uint32_t* wires;  // c columns of n values, column j at + 8 j stride words
    const uint32_t* table;  // c resident columns of n values, column j at + 8 j n words
    const uint32_t* qk;     // n values
    uint32_t n, c;
    size_t stride;
    Fr30 k14;                    // 2^(270 + 14)
    Fr30 theta[kPqMaxColumns];   // theta^j, multipliers
};

__global__ void __launch_bounds__(kPqTile) k_lk_fold(LkFoldArgs in, uint32_t* __restrict__ out_f, uint32_t* __restrict__ out_t) {
    const uint32_t i = blockIdx.x * kPqTile + threadIdx.x;
    if (i >= in.n) return;
    const Fr30 sf = lk_folded(in.wires + 8 * (size_t)i, in.stride, in.c, in.theta);
    fr30_store(out_f + 8 * (size_t)i, fr30_mul(fr30_mul(sf, fr30_load(in.qk + 8 * (size_t)i)), in.k14));
    const Fr30 st = lk_folded(in.table + 8 * (size_t)i, in.n, in.c, in.theta);
    fr30_store(out_t + 8 * (size_t)i, fr30_sum_reduce(st));
}

struct LkArgs {
    const uint32_t* wires;  // c columns of N values, column j at + 8 j stride words (the call's workspace)
    const uint32_t* table;  // c resident columns of N values, column j at + 8 j N words
    const uint32_t* qk;     // N values each
    const uint32_t* l0;
    const uint32_t* mult;
    const uint32_t* phi;
    uint32_t log_N, rot, c;
    size_t stride;
    Fr30 beta;                   // image
    Fr30 k14, ak14, a3;          // 2^(270 + 14), alpha 2^(270 + 14), alpha^3 2^270
    Fr30 theta[kPqMaxColumns];   // theta^j, multipliers
};

__global__ void __launch_bounds__(kPqTile) k_lk_constraints(LkArgs in, uint32_t* __restrict__ out) {
    const uint32_t N = 1u << in.log_N;
    const uint32_t i = blockIdx.x * kPqTile + threadIdx.x;
    if (i >= N) return;
    const uint32_t ir = (i + in.rot) & (N - 1);
    const Fr30 sf = lk_folded(in.wires + 8 * (size_t)i, in.stride, in.c, in.theta);
    const Fr30 F = fr30_add(in.beta, fr30_mul(fr30_mul(sf, fr30_load(in.qk + 8 * (size_t)i)), in.k14));
    const Fr30 Tt = fr30_add(in.beta, lk_folded(in.table + 8 * (size_t)i, (size_t)N, in.c, in.theta));  // an operand only
    const Fr30 phi = fr30_load(in.phi + 8 * (size_t)i);
    const Fr30 D = fr30_sub(fr30_load(in.phi + 8 * (size_t)ir), phi);
    const Fr30 E = fr30_add(fr30_load(in.mult + 8 * (size_t)i), fr30_mul(fr30_mul(D, Tt), in.k14));
    Fr30 W = fr30_sub(fr30_mul(fr30_mul(E, F), in.k14), Tt);                                              // Lk1
    W = fr30_add(W, fr30_mul(fr30_mul(fr30_load(in.l0 + 8 * (size_t)i), phi), in.ak14));                  // + alpha Lk2: an operand only
    fr30_store(out + 8 * (size_t)i, fr30_mul(W, in.a3));
}

}  // namespace

void launch_lk_fold(hipStream_t s, const uint32_t* d_wires, size_t stride, const uint32_t* d_table, const uint32_t* d_qk, uint32_t n,
                    uint32_t c, const LkScalars& sc, uint32_t* d_out_f, uint32_t* d_out_t) {
    LkFoldArgs in{};
    in.wires = d_wires;
    in.table = d_table;
    in.qk = d_qk;
    in.n = n;
    in.c = c;
    in.stride = stride;
    in.k14 = *sc.k14;
    for (uint32_t j = 0; j < c && j < kPqMaxColumns; j++) in.theta[j] = sc.theta[j];
    hipLaunchKernelGGL(k_lk_fold, dim3((n + kPqTile - 1) / kPqTile), dim3(kPqTile), 0, s, in, d_out_f, d_out_t);
}

void launch_lk_constraints(hipStream_t s, const LkColumns& cols, uint32_t log_N, uint32_t rot, uint32_t c, size_t stride,
                           const LkScalars& sc, uint32_t* d_out) {
    LkArgs in{};
    in.wires = cols.d_wires;
    in.table = cols.d_table;
    in.qk = cols.d_qk;
    in.l0 = cols.d_l0;
    in.mult = cols.d_mult;
    in.phi = cols.d_phi;
    in.log_N = log_N;
    in.rot = rot;
    in.c = c;
    in.stride = stride;
    in.beta = *sc.beta;
    in.k14 = *sc.k14;
    in.ak14 = *sc.ak14;
    in.a3 = *sc.a3;
    for (uint32_t j = 0; j < c && j < kPqMaxColumns; j++) in.theta[j] = sc.theta[j];
    const uint32_t N = 1u << log_N;
    hipLaunchKernelGGL(k_lk_constraints, dim3((N + kPqTile - 1) / kPqTile), dim3(kPqTile), 0, s, in, d_out);
}

}  // namespace kzg
