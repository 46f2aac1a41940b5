// custom_gate_kernels.hip -- the custom gates of a circuit whose key holds selector x wire-monomial terms: their sum on the coset,
// the caller's term of the quotient's numerator (kzg_circuit_custom_gate, kzg_circuit_custom_quotient, kzg_circuit_custom_prove;
// DESIGN.md section 4.27).
//
// Domain, coset and notation are circuit_kernels.hip's: n = 2^k, N = rot n, x_i = g w_N^i.  A custom circuit keeps g <= 8 selector
// columns qx_s beside the key of section 4.22 and an exponent matrix p[s][j] in 0..7 (g x t bytes, row-major), d_s = sum_j p[s][j]
// >= 1.  With the wire columns f_j:
//
//     G'    = sum_{s<g} qx_s prod_{j<t} f_j^p[s][j]                                                  (on the coset: k_cg_gate)
//
// Kernel (one coset point per lane, kPqTile = 256 lanes per workgroup, the loops over terms, wires and exponents not unrolled: their
// trip counts are the kernel's arguments, uniform over the launch; nothing intermediate stored):
//   k_cg_gate   N lanes: point i of the extended wires (the call's workspace, column j at + 8 j stride words) and of the resident
//               coset forms of the qx_s (column s at + 8 s N words) -> G'_i, written where k_ck_constraints reads its caller's term.
//               A wire is read once per term that uses it (exponent 0: not read); the second read of a term comes from the cache.
//
// Forms (fr30.hip.h; fr30_mul(a, b) = a b / 2^270; IMAGE = x 2^256, MULTIPLIER = x 2^270).  Every column is stored as images.
//   W_j = f_j k14              image x k14, k14 = 2^(270 + 14) in multiplier form: f_j 2^270, the MULTIPLIER form of the wire.
//   A_0 = qx_s                 the selector's image.
//   A_(k+1) = A_k W_j          image x multiplier = image: p[s][j] times for every wire j; A_(d_s) is the IMAGE of term s.
//   S = sum_s A_(d_s)          images, one carry pass per addition (fr30_add).
//   G'_i = S x one             one = 2^270: the value unchanged, the magnitude reduced (fr30_sum_reduce); stored canonical.
//
// Bounds.  A loaded value is canonical, [0, r), in carry-normalised digits (0..7 within [-2^29 - 4, 2^29 + 4], top digit at most
// 0x73ee).  A product returns |v| <= 0.5001 r + |a b| / 2^270 with digits 0..7 in [-2^29, 2^29); r^2 / 2^270 < r / 2^15.
//   W_j           canonical x canonical k14: |v| < 0.5002 r, top digit below 0.5002 x 0x73ee + 1 < 2^14.
//   A_0           canonical, [0, r).
//   A_(k+1)       |A_k| < r and |W_j| < 0.5002 r: |v| <= 0.5001 r + 0.5002 r^2 / 2^270 < 0.5002 r, by induction for every k >= 1.
//                 Both operands of every product have digits 0..7 within 2^29 + 4 and a top digit below 2^15: a column is at most
//                 9 x (2^29 + 4)^2 + 3.7 x 2^58 < 2^62, inside what fr30_mul takes.  d_s >= 1: a term is always a product.
//   S             zero, then g <= 8 terms of |v| < 0.5002 r, each added with its own carry pass (one product's digits, within 2^29,
//                 on normalised digits, within 2^29 + 4: raw digits within 2^30 + 4 < 2^31 - 2^29, what fr30_norm asks for):
//                 |S| < 8 x 0.5002 r < 4.002 r, normalised digits 0..7, top digit below 4.002 x 0x73ee + 1 < 2^17.  Outside what
//                 fr30_to_limbs takes ((-r, 2 r)): never stored, the operand of the last product only.
//   S x one       |one270| < r / 2 in balanced digits: a column is at most 8 x (2^29 + 4) x 2^29 + 2^17 x 2^29 + 3.7 x 2^58 < 2^62;
//                 |v| <= 0.5001 r + 4.002 r (r / 2) / 2^270 < 0.5002 r, stored through fr30_to_limbs.
// No zero test is made: an unsatisfied gate shows in the quotient's remainder.
// Indices: i < N <= 2^22; every column offset (8 j stride + 8 i words, 8 s N + 8 i words) is formed in 64 bits.  The exponent
// matrix is read at s t + j < 8 x 7 = kCgMaxTerms x kPqMaxColumns, the size of its array in the arguments.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "fr30.hip.h"
#include "fr30_lanes.hip.h"

namespace kzg {

namespace {

static_assert(kPqTile == 256, "one coset point per lane of a 256-lane workgroup");

struct CgArgs {
    const uint32_t* wires;  // t columns of N values, column j at + 8 j stride words (the call's workspace)
    const uint32_t* qx;     // g resident columns of N values, column s at + 8 s N words
    uint32_t N, t, g;
    size_t stride;
    Fr30 k14;                                      // 2^(270 + 14)
    uint8_t exps[kCgMaxTerms * kPqMaxColumns];     // p[s][j] at s t + j
};

__global__ void __launch_bounds__(kPqTile) k_cg_gate(CgArgs in, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * kPqTile + threadIdx.x;
    if (i >= in.N) return;
    const uint32_t* q = in.qx + 8 * (size_t)i;
    Fr30 sum = fr30_zero();
#pragma unroll 1
    for (uint32_t s = 0; s < in.g; s++) {
        Fr30 acc = fr30_load(q);
        q += 8 * (size_t)in.N;
        const uint32_t* w = in.wires + 8 * (size_t)i;
#pragma unroll 1
        for (uint32_t j = 0; j < in.t; j++) {
            const uint32_t p = in.exps[s * in.t + j];
            if (p) {
                const Fr30 W = fr30_mul(fr30_load(w), in.k14);
#pragma unroll 1
                for (uint32_t k = 0; k < p; k++) acc = fr30_mul(acc, W);
            }
            w += 8 * in.stride;
        }
        sum = fr30_add(sum, acc);
    }
    fr30_store(out + 8 * (size_t)i, fr30_sum_reduce(sum));  // (sum: an operand only)
}

}  // namespace

void launch_cg_gate(hipStream_t s, const uint32_t* d_wires, size_t stride, const uint32_t* d_qx, uint32_t N, uint32_t t, uint32_t g,
                    const uint8_t* exps, const Fr30& k14, uint32_t* d_out) {
    CgArgs in{};
    in.wires = d_wires;
    in.qx = d_qx;
    in.N = N;
    in.t = t < kPqMaxColumns ? t : kPqMaxColumns;
    in.g = g < kCgMaxTerms ? g : kCgMaxTerms;
    in.stride = stride;
    in.k14 = k14;
    for (uint32_t k = 0; k < in.g * in.t; k++) in.exps[k] = exps[k] & 7;
    hipLaunchKernelGGL(k_cg_gate, dim3((N + kPqTile - 1) / kPqTile), dim3(kPqTile), 0, s, in, d_out);
}

}  // namespace kzg
