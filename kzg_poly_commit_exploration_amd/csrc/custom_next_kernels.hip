// custom_next_kernels.hip -- the custom gates of a next-row circuit: selector x wire-monomial terms whose factors are read at the
// row and at the row after it (kzg_circuit_custom_next_gate, kzg_circuit_custom_next_quotient, kzg_circuit_custom_next_prove;
// DESIGN.md section 4.28).  The sibling of custom_gate_kernels.hip, in a unit of its own so that k_cg_gate compiles to what it did.
//
// Domain, coset and notation are circuit_kernels.hip's: n = 2^k, N = e n, x_i = g w_N^i, w = w_N^e the root of the domain H.  A
// next-row circuit keeps, beside the g <= 8 selector columns qx_s and the exponents p[s][j] of section 4.27, a second matrix
// p'[s][j] in 0..7 (g x t bytes, row-major), d_s = sum_j (p[s][j] + p'[s][j]) >= 1.  With the wire columns f_j:
//
//     G'(X) = sum_{s<g} qx_s(X) prod_{j<t} f_j(X)^p[s][j] prod_{j<t} f_j(w X)^p'[s][j]               (on the coset: k_cgn_gate)
//
// On the coset w x_i = g w_N^(i + e) = x_((i + e) mod N): f_j(w x_i) is the extended wire column at index (i + e) mod N, no new
// transform.
//
// Kernel (one coset point per lane, kPqTile = 256 lanes per workgroup, the loops over terms, wires and exponents not unrolled: their
// trip counts are the kernel's arguments, uniform over the launch; nothing intermediate stored):
//   k_cgn_gate  N lanes: k_cg_gate's reads, and for every (term, wire) with p'[s][j] > 0 the wire at index (i + e) mod N, a plain
//               second load: lane i + e of the launch loads the same 32 bytes as its own point, so the line is in the cache or
//               on its way.  The wrapped index is formed per lane: i + e < 2^23, reduced by one conditional subtraction (e <= N).
//               N < 256: the wrap falls inside the one partial workgroup; N a multiple of 256: the last e lanes of the last one.
//               G'_i is written where k_ck_constraints reads its caller's term.
//
// Forms and bounds are k_cg_gate's, operand by operand (fr30.hip.h; fr30_mul(a, b) = a b / 2^270; IMAGE = x 2^256, MULTIPLIER =
// x 2^270); the helpers are the same and are called in the same order, so tests/host/cg_reach_host.cpp, which replays that order
// at the bounds' edge, covers this kernel's arithmetic: which row a factor was loaded from changes an address, not a magnitude.
//   W_j, W'_j     canonical wire (row i, row i + 1) x canonical k14: |v| < 0.5002 r, top digit below 2^14.
//   A_0           the selector's image, canonical, [0, r).
//   A_(k+1)       A_k W_j or A_k W'_j: |A_k| < r and |W| < 0.5002 r give |v| <= 0.5001 r + 0.5002 r^2 / 2^270 < 0.5002 r, by
//                 induction for every k >= 1, whichever row the factor came from.  Both operands of every product have digits 0..7
//                 within 2^29 + 4 and a top digit below 2^15: a column is at most 9 x (2^29 + 4)^2 + 3.7 x 2^58 < 2^62, inside
//                 what fr30_mul takes.  d_s >= 1: a term is always a product; d_s <= 7 only bounds the trip count.
//   S             zero, then g <= 8 terms of |v| < 0.5002 r, each added with its own carry pass (fr30_add): |S| < 4.002 r, top
//                 digit below 2^17; never stored, the operand of the last product only.
//   S x one       fr30_sum_reduce: a column is at most 8 x (2^29 + 4) x 2^29 + 2^17 x 2^29 + 3.7 x 2^58 < 2^62;
//                 |v| <= 0.5001 r + 4.002 r (r / 2) / 2^270 < 0.5002 r, stored through fr30_to_limbs.
// No zero test is made: an unsatisfied gate shows in the quotient's remainder.
// Indices: i < N <= 2^22, e <= 2^4: i + e does not wrap 32 bits and (i + e) mod N < N; every column offset (8 j stride + 8 i words,
// 8 s N + 8 i words) is formed in 64 bits.  Both matrices are read at s t + j < 8 x 7 = kCgMaxTerms x kPqMaxColumns, the size of
// their arrays in the arguments.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "fr30.hip.h"
#include "fr30_lanes.hip.h"

namespace kzg {

namespace {

static_assert(kPqTile == 256, "one coset point per lane of a 256-lane workgroup");

struct CgnArgs {
    const uint32_t* wires;  // t columns of N values, column j at + 8 j stride words (the call's workspace)
    const uint32_t* qx;     // g resident columns of N values, column s at + 8 s N words
    uint32_t N, t, g, e;    // e: the distance of the next row on the coset, N / n
    size_t stride;
    Fr30 k14;                                      // 2^(270 + 14)
    uint8_t exps[kCgMaxTerms * kPqMaxColumns];     // p[s][j] at s t + j
    uint8_t next[kCgMaxTerms * kPqMaxColumns];     // p'[s][j] at s t + j
};

__global__ void __launch_bounds__(kPqTile) k_cgn_gate(CgnArgs in, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * kPqTile + threadIdx.x;
    if (i >= in.N) return;
    uint32_t i1 = i + in.e;  // (i + e) mod N, per lane
    if (i1 >= in.N) i1 -= in.N;
    const uint32_t* q = in.qx + 8 * (size_t)i;
    Fr30 sum = fr30_zero();
#pragma unroll 1
    for (uint32_t s = 0; s < in.g; s++) {
        Fr30 acc = fr30_load(q);
        q += 8 * (size_t)in.N;
        const uint32_t* w = in.wires;
#pragma unroll 1
        for (uint32_t j = 0; j < in.t; j++) {
            const uint32_t p = in.exps[s * in.t + j], pn = in.next[s * in.t + j];
            if (p) {
                const Fr30 W = fr30_mul(fr30_load(w + 8 * (size_t)i), in.k14);
#pragma unroll 1
                for (uint32_t k = 0; k < p; k++) acc = fr30_mul(acc, W);
            }
            if (pn) {
                const Fr30 W = fr30_mul(fr30_load(w + 8 * (size_t)i1), in.k14);
#pragma unroll 1
                for (uint32_t k = 0; k < pn; k++) acc = fr30_mul(acc, W);
            }
            w += 8 * in.stride;
        }
        sum = fr30_add(sum, acc);
    }
    fr30_store(out + 8 * (size_t)i, fr30_sum_reduce(sum));  // (sum: an operand only)
}

}  // namespace

void launch_cgn_gate(hipStream_t s, const uint32_t* d_wires, size_t stride, const uint32_t* d_qx, uint32_t N, uint32_t e, uint32_t t,
                     uint32_t g, const uint8_t* exps, const uint8_t* exps_next, const Fr30& k14, uint32_t* d_out) {
    CgnArgs in{};
    in.wires = d_wires;
    in.qx = d_qx;
    in.N = N;
    in.t = t < kPqMaxColumns ? t : kPqMaxColumns;
    in.g = g < kCgMaxTerms ? g : kCgMaxTerms;
    in.e = e < N ? e : 0;  // (e = N / n and n >= 2; anything else reads the row itself, never out of bounds)
    in.stride = stride;
    in.k14 = k14;
    for (uint32_t k = 0; k < in.g * in.t; k++) {
        in.exps[k] = exps[k] & 7;
        in.next[k] = exps_next[k] & 7;
    }
    hipLaunchKernelGGL(k_cgn_gate, dim3((N + kPqTile - 1) / kPqTile), dim3(kPqTile), 0, s, in, d_out);
}

}  // namespace kzg
