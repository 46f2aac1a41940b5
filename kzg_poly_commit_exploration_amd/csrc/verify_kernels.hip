// verify_kernels.hip -- one random-linear-combination check of many cell proofs (kzg_verify_cells_batch,
// kzg_verify_cells_lincomb).
//
// Records t = (commitment b_t, cell j_t, values v_t, proof pi_t), weights rho_t, a_j = w_M^j.  The two G1 sides are
//     LHS = sum_t rho_t pi_t = sum_j T_j,        T_j = sum_{t: j_t = j} rho_t pi_t
//     RHS = sum_b [U_b] C_b - [A(s)]G1 + sum_j [a_j] T_j,    U_b = sum_{t: b_t = b} rho_t,   A = sum_t rho_t I_t
// and the host checks e(LHS, [s^l]G2) == e(RHS, G2).  The host sorts the records by cell id (order[t'] = the record at
// sorted position t') and plans every segmented sum as levels of groups of at most kVcFold consecutive entries of one
// segment, so no lane adds more than kVcFold - 1 terms per level whatever the distribution of the ids.
//
// Kernels:
//   k_vc_ladder     lane per point: proofs and commitments (from the normalised upload) are checked to lie on the curve
//                   and in G1 (Scott, ePrint 2021/1130: [z^2] P == (beta^2 x, -y), i.e. phi'(P) = [-z^2] P for the cube
//                   root beta^2 = -1 - beta), then multiplied by their weight with g1_mul_glv: a + b lambda with 64-bit
//                   a, b for the proofs (64 joint steps; the ladder of fk20_kernels.hip), a split full scalar for the commitments and the SRS terms of
//                   -[A(s)] (128).  [z^2] P runs as two ladders of |z| in the same loop as the weight, one copy of it.
//   k_vc_cell_scale [a_j] T_j, a_j from the context's split twiddles (Glv), 128 joint steps
//   k_vc_g1_sum     one level of a segmented sum of XYZZ records (T_j; the two sides at the end)
//   k_vc_fr_sum     one level of a segmented sum of rows of l Fr values; the first level gathers the rows in sorted order
//                   and multiplies them by the weights: V_j[i] = sum_{t: j_t = j} rho_t v_t[i]
//   k_vc_fr_twist   after the batched inverse transforms of the V_j (k_fr_stage): x h_j^-i / l, h_j = w_N^j, so that
//                   the column sums are the coefficients of A
//
// Bounds: the group law of g1_30.hip.h on its own outputs and on normalised points (section 4.2); Fr values as in
// recover_kernels.hip: canonical in and out, a product |v| <= 0.5002 r, a running sum of at most kVcFold such values or
// canonical ones (fr30_add keeps the digits carry-normalised, |sum| < 2^260) is brought back below r by one product with
// the multiplier form of one before it is stored.
#define KZG_G1_30_INLINE_DBL
#define KZG_G1_30_NO_SB
#include <hip/hip_runtime.h>

#include "engine.h"
#include "fr30.hip.h"
#include "fr30_lanes.hip.h"
#include "g1_30.hip.h"

namespace kzg {

namespace {

// fk20_kernels.hip's GLV ladder, restated here (both live in anonymous namespaces of their translation units):
// beta * 2^390 mod p, balanced radix-2^30 digits: the cube root of unity with (beta x, y) = [z^2 - 1](x, y) on G1
// (the same digits as fk20_kernels.hip, tests/test_verify_cells.py compares them)
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

constexpr uint32_t kVcThreads = 64;
constexpr uint32_t kVcFrThreads = 256;
constexpr uint64_t kBlsZAbs = 0xd201000000010000ULL;  // |z|, z = -0xd201000000010000

__device__ __forceinline__ Fq fq_four() {
    const Fq one = fq_one();
    const Fq two = fq_norm(fq_add_raw(one, one));  // one carry pass per doubling: four raw digits could pass 2^31
    return fq_norm(fq_add_raw(two, two));
}
// a == b * c for lazily reduced values below 3.5 p after the subtraction
__device__ __forceinline__ bool fq_eq_prod(const Fq& a, const Fq& b, const Fq& c) {
    return fq_is_zero(fq_norm(fq_sub_raw(a, fq_mul(b, c))));
}

// lane t < lanes: the point rec[src ? src[t] : t]; lanes t < n_check are checked first (err[0]: least failing index off
// the curve, err[1]: least failing index outside G1; such a lane writes infinity).  [glv[t]] P goes to out_a[t] for
// t < split, else out_b[t - split].
__global__ void __launch_bounds__(kVcThreads) k_vc_ladder(const uint4* __restrict__ rec, const uint32_t* __restrict__ src,
                                                          const Glv* __restrict__ glv, uint32_t lanes, uint32_t n_check,
                                                          uint32_t split, uint4* __restrict__ out_a, uint4* __restrict__ out_b,
                                                          uint32_t* __restrict__ err) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= lanes) return;
    const uint32_t idx = src ? src[t] : t;
    const uint4* r = rec + (size_t)idx * kAffineU4;
    Affine30 p;
    p.x = load_fq16(r);
    p.y = load_fq16(r + 4);
    uint4* o = t < split ? out_a + (size_t)t * kXyzzU4 : out_b + (size_t)(t - split) * kXyzzU4;
    XYZZ30 base = xyzz30_inf();
    if (!affine30_is_inf(p)) {
        base.X = p.x;
        base.Y = p.y;
        base.ZZ = fq_one();
        base.ZZZ = base.ZZ;
    }
    const bool check = t < n_check && !xyzz30_is_inf(base);
    if (check && !fq_is_zero(fq_norm(fq_sub_raw(fq_sub_raw(fq_sqr(p.y), fq_mul(fq_sqr(p.x), p.x)), fq_four())))) {
        atomicMin(err, idx);
        store_xyzz30(o, xyzz30_inf());
        return;
    }
    const Glv w = load_glv(glv, t);
    // rounds 0, 1: q = [|z|] q twice, from P (checked lanes only); round 2: [w] P.  Operands selected field by field, so
    // that nothing is addressed through memory.
    XYZZ30 q = base;
#pragma unroll 1
    for (int round = check ? 0 : 2; round < 3; round++) {
        const bool z_round = round < 2;
        Glv k;
        k.k1[0] = z_round ? kBlsZAbs : w.k1[0];
        k.k1[1] = z_round ? 0 : w.k1[1];
        k.k2[0] = z_round ? 0 : w.k2[0];
        k.k2[1] = z_round ? 0 : w.k2[1];
        if (!z_round) q = base;
        q = g1_mul_glv(q, k);
        if (round == 1) {
            // [z^2] P == (beta^2 x, -y) with beta^2 = -1 - beta: X == -(x + beta x) ZZ and Y == -y ZZZ
            const Fq ex = fq_norm(fq_neg(fq_norm(fq_add_raw(p.x, fq_mul(p.x, fq_beta())))));
            const bool in_g1 = !xyzz30_is_inf(q) && fq_eq_prod(q.X, ex, q.ZZ) && fq_eq_prod(q.Y, fq_neg(p.y), q.ZZZ);
            if (!in_g1) {
                atomicMin(err + 1, idx);
                store_xyzz30(o, xyzz30_inf());
                return;
            }
        }
    }
    store_xyzz30(o, q);
}

// out[d] = [a_(ids[d])] T[d], a_j = w_M^j = tw[j << shift] (split twiddles)
__global__ void __launch_bounds__(kVcThreads) k_vc_cell_scale(const uint4* __restrict__ T, const uint32_t* __restrict__ ids,
                                                              uint32_t D, const Glv* __restrict__ tw, uint32_t shift,
                                                              uint4* __restrict__ out) {
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    store_xyzz30(out + (size_t)d * kXyzzU4, g1_mul_glv(load_xyzz30(T + (size_t)d * kXyzzU4), load_glv(tw, ids[d] << shift)));
}

// out[g] = sum of in[starts[g] .. starts[g + 1])
__global__ void __launch_bounds__(kVcThreads) k_vc_g1_sum(const uint4* __restrict__ in, const uint32_t* __restrict__ starts,
                                                          uint32_t groups, uint4* __restrict__ out) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= groups) return;
    const uint32_t s0 = starts[g], s1 = starts[g + 1];
    XYZZ30 acc = load_xyzz30(in + (size_t)s0 * kXyzzU4);
#pragma unroll 1
    for (uint32_t i = s0 + 1; i < s1; i++) xyzz30_add(acc, load_xyzz30(in + (size_t)i * kXyzzU4));
    store_xyzz30(out + (size_t)g * kXyzzU4, acc);
}

// lane (g, i): out[g l + i] = sum over rows q in [starts[g], starts[g + 1]) of in[q' l + i] (x rho[q]), where q' = order[q]
// when the rows are weighted (rho != null) and q otherwise
__global__ void __launch_bounds__(kVcFrThreads) k_vc_fr_sum(const uint32_t* __restrict__ in, const uint32_t* __restrict__ order,
                                                            const Fr30* __restrict__ rho, const uint32_t* __restrict__ starts,
                                                            uint64_t lanes, uint32_t log_l, uint32_t* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= lanes) return;
    const uint32_t g = (uint32_t)(t >> log_l), i = (uint32_t)t & ((1u << log_l) - 1);
    const uint32_t s0 = starts[g], s1 = starts[g + 1];
    Fr30 acc = fr30_zero();
#pragma unroll 1
    for (uint32_t q = s0; q < s1; q++) {
        const uint32_t row = rho ? order[q] : q;
        Fr30 v = fr30_load(in + 8 * (((uint64_t)row << log_l) + i));
        if (rho) v = fr30_mul(v, fr30_table(rho, q));
        acc = fr30_add(acc, v);
    }
    fr30_store(out + 8 * t, fr30_mul(acc, fr30_const_one270()));
}

// lane (d, i): io[d l + i] x w_N^-(ids[d] i) / l; itw: the inverse NTT twiddles (lo / hi tables of w_(2^22)^-e)
__global__ void __launch_bounds__(kVcFrThreads) k_vc_fr_twist(uint32_t* __restrict__ io, const uint32_t* __restrict__ ids,
                                                              const Fr30* __restrict__ itw, uint32_t log_n, uint32_t log_l,
                                                              uint64_t lanes, Fr30 inv_l) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= lanes) return;
    const uint32_t d = (uint32_t)(t >> log_l), i = (uint32_t)t & ((1u << log_l) - 1);
    const uint32_t e = ((ids[d] * i) & ((1u << log_n) - 1)) << (kNttMaxLog - log_n);
    const Fr30 m = fr30_mul(fr30_mul(fr30_table(itw + kNttTableLen, e >> 11), fr30_table(itw, e & (kNttTableLen - 1))), inv_l);
    fr30_store(io + 8 * t, fr30_mul(fr30_load(io + 8 * t), m));
}

dim3 vc_grid(uint64_t lanes, uint32_t threads) { return dim3((unsigned)((lanes + threads - 1) / threads)); }

}  // namespace

void launch_vc_ladder(hipStream_t s, const void* d_rec, const uint32_t* d_src, const Glv* d_glv, uint32_t lanes, uint32_t n_check,
                      uint32_t split, void* d_out_a, void* d_out_b, uint32_t* d_err) {
    if (!lanes) return;
    hipLaunchKernelGGL(k_vc_ladder, vc_grid(lanes, kVcThreads), dim3(kVcThreads), 0, s, (const uint4*)d_rec, d_src, d_glv, lanes,
                       n_check, split, (uint4*)d_out_a, (uint4*)d_out_b, d_err);
}

void launch_vc_cell_scale(hipStream_t s, const void* d_T, const uint32_t* d_ids, uint32_t D, const Glv* d_tw, uint32_t shift,
                          void* d_out) {
    if (!D) return;
    hipLaunchKernelGGL(k_vc_cell_scale, vc_grid(D, kVcThreads), dim3(kVcThreads), 0, s, (const uint4*)d_T, d_ids, D, d_tw, shift,
                       (uint4*)d_out);
}

void launch_vc_g1_sum(hipStream_t s, const void* d_in, const uint32_t* d_starts, uint32_t groups, void* d_out) {
    if (!groups) return;
    hipLaunchKernelGGL(k_vc_g1_sum, vc_grid(groups, kVcThreads), dim3(kVcThreads), 0, s, (const uint4*)d_in, d_starts, groups,
                       (uint4*)d_out);
}

void launch_vc_fr_sum(hipStream_t s, const uint32_t* d_in, const uint32_t* d_order, const Fr30* d_rho, const uint32_t* d_starts,
                      uint32_t groups, uint32_t log_l, uint32_t* d_out) {
    const uint64_t lanes = (uint64_t)groups << log_l;
    if (!lanes) return;
    hipLaunchKernelGGL(k_vc_fr_sum, vc_grid(lanes, kVcFrThreads), dim3(kVcFrThreads), 0, s, d_in, d_order, d_rho, d_starts, lanes,
                       log_l, d_out);
}

void launch_vc_fr_twist(hipStream_t s, uint32_t* d_io, const uint32_t* d_ids, uint32_t D, const void* d_itw, uint32_t log_n,
                        uint32_t log_l, const Fr30& inv_l) {
    const uint64_t lanes = (uint64_t)D << log_l;
    if (!lanes) return;
    hipLaunchKernelGGL(k_vc_fr_twist, vc_grid(lanes, kVcFrThreads), dim3(kVcFrThreads), 0, s, d_io, d_ids, (const Fr30*)d_itw,
                       log_n, log_l, lanes, inv_l);
}

}  // namespace kzg
