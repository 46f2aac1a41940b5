// circuit_verify_kernels.hip -- the second stage of the batch verifier of circuit proofs (kzg_circuit_verify_proofs_batch,
// kzg_circuit_verify_proofs_lincomb).
//
// Proof k of a batch contributes, with its weight rho_k and its challenge zeta_k (w: the root of the circuit's domain),
//     P0 += [-zeta_k w] D_k + [-zeta_k] E_k + [-zeta_k^2 w] F_k
//     P1 +=             D_k +            E_k + [zeta_k (1 + w)] F_k
//     P2 -=                                                     F_k
// where the first stage (k_vc_ladder and k_vc_g1_sum of verify_kernels.hip, through their launchers) has left
//     D_k = rho_k (the proof's own points of A_0k), E_k = [rho_k v_k^(2t)][z_k], F_k = [rho_k] W_k
// as XYZZ records.  The scalars differ from proof to proof, so they come as one split record (Glv) per product where
// k_vc_cell_scale indexes a table of twiddles.
//
// Kernels:
//   k_cvb_public    PI(zeta_k) = (zeta_k^n - 1) / n sum_(i < n_public) PI_k,i w^i / (zeta_k - w^i) for every proof: one workgroup of
//                   64 lanes per proof, lane t takes the rows t, t + 64, ..; the 64 denominators of a round are inverted together
//                   (cvb_group_inverse: a product scan from both ends in LDS and ONE fr30_inv per workgroup, as
//                   bary_kernels.hip does).  zeta_k = w^i puts one in the denominator's place, records i and returns PI_k,i.
//   k_cvb_lin       one lane per proof: zeta^n, L_0(zeta) (the 64 proofs of a workgroup share one inversion; zeta = 1 puts one in
//                   its place and L_0 = 1), A, B and the three scalars of lin_scalars that need them: [z]'s, sigma_(t-1)'s, the
//                   constant.  Four values a proof, for k_cvb_scalars.
//   k_cvb_scalars   one lane per scalar that leaves: the others of lin_scalars and custom_lin_scalars (from the exponent matrix),
//                   all times rho_k, v_k^i and the stage-2 factors.  Per proof the split scalars (Glv) of its own t + e + 1
//                   products of stage 1 and of its four of stage 2, and its row of 2 (2t + 3 + g) key-side terms, which
//                   k_vc_fr_sum then sums over the proofs.  (One lane per proof for all of it does not fit the register file.)
//   k_cvb_key_split the 2 (2t + 3 + g) sums of the key side, split for the ladder
//   k_cvb_stage2    lane (k, j), j < 4: one 128-step GLV ladder, [s_(k,j)] X with X = D_k, E_k, F_k, F_k.  The products j < 3
//                   are proof k's three terms of P0, product 3 is its third term of P1.  D_k and E_k are terms of P1 and F_k
//                   is a term of P2 (whose sum the host negates) as the first stage left them, so nothing is copied: the host
//                   lays the records out so that k_vc_g1_sum sums every side, the key's terms included, over consecutive records.
//
// Forms (fr30.hip.h): inputs are blst_fr images (x 2^256), canonical: the challenges, the weights, the evaluations as
// k_wire_fr decoded them, the public inputs.  One product with 2^284 (consts[0]) takes an image into the multiplier form
// x 2^270, in which everything is computed: a product of two multipliers is a multiplier.  A value leaves as the plain integer
// x = fr30_to_limbs(fr30_mul(v, 1)), canonical, which is what glv_split_device and the rows of k_vc_fr_sum take.
// Bounds: every product returns |v| <= 0.5001 r + |a b| / 2^270 and takes carry-normalised digits (one operand may be a raw sum of
// two).  Every sum here is carry-normalised (fr30_add, fr30_sub) and has at most 2t + 3 <= 17 terms of magnitude <= 0.5001 r
// (t <= kPqMaxColumns = 7; g0 + g1, the constant of G1: the three terms of r's constant, 2t - 1 subtractions, g1) before it feeds a
// product: below 8.6 r < 2^258, far inside |a| |b| < 2^528 and the top digit's 2^30.  The custom terms (g <= kCgMaxTerms) are
// products only.  A negation is digit-wise and keeps the digit bounds, which are symmetric.  PI's running sum is brought back under
// 0.51 r by a product with the multiplier form of one after every term; the 64 lanes' totals add to less than 32.7 r < 2^260.  Zero
// tests are made on the canonical residue of a value first reduced by such a product, so that fr30_to_limbs sees a value inside
// (-r, 2r): a lazy difference of two products lies in (-1.0002 r, 1.0002 r) and may hold r, or -r, for zero (its operands the two
// representatives of a residue next to r / 2; a product's own operands decide which one it returns), and it passes -r when it is
// not zero.  The split scalars are plain integers below r < 2^255.  tests/host/cvb_reach_host.cpp replays these kernels on the
// host at those magnitudes.
// G1: the group law of g1_30.hip.h on its own outputs (section 4.2): the inputs of k_cvb_stage2 are what k_vc_ladder and
// k_vc_g1_sum stored, the ladder is verify_kernels.hip's and its outputs go to k_vc_g1_sum, as k_vc_cell_scale's do.
#define KZG_G1_30_INLINE_DBL
#define KZG_G1_30_NO_SB
#include <hip/hip_runtime.h>

#include "engine.h"
#include "fr30.hip.h"
#include "fr30_lanes.hip.h"
#include "g1_30.hip.h"

namespace kzg {

namespace {

// verify_kernels.hip's GLV ladder, restated here (both live in anonymous namespaces of their translation units):
// beta * 2^390 mod p, balanced radix-2^30 digits: the cube root of unity with (beta x, y) = [z^2 - 1](x, y) on G1
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

constexpr uint32_t kCvbThreads = 64;

// ---- the Fr side -------------------------------------------------------------------------------------------------------------
// srs_update_kernels.hip's split, restated here: the canonical scalar k (8 x u32, below r) as k1 + k2 lambda, k1 = k mod lambda,
// k2 = k div lambda, lambda = z^2 - 1 -- the host's glv_split, a restoring division bit by bit
constexpr uint64_t kLambdaHi = 0xac45a4010001a402ULL, kLambdaLo = 0x00000000ffffffffULL;
__device__ __forceinline__ Glv glv_split_device(const uint32_t l[8]) {
    uint64_t v0 = l[0] | ((uint64_t)l[1] << 32), v1 = l[2] | ((uint64_t)l[3] << 32), v2 = l[4] | ((uint64_t)l[5] << 32),
             v3 = l[6] | ((uint64_t)l[7] << 32);
    uint64_t r0 = 0, r1 = 0, q0 = 0, q1 = 0;
#pragma unroll 1
    for (int bit = 0; bit < 256; bit++) {
        const bool over = (r1 >> 63) != 0;  // the remainder shifted left passes 2^128: it is above lambda then
        r1 = (r1 << 1) | (r0 >> 63);
        r0 = (r0 << 1) | (v3 >> 63);
        v3 = (v3 << 1) | (v2 >> 63);
        v2 = (v2 << 1) | (v1 >> 63);
        v1 = (v1 << 1) | (v0 >> 63);
        v0 <<= 1;
        q1 = (q1 << 1) | (q0 >> 63);
        q0 <<= 1;
        if (over || r1 > kLambdaHi || (r1 == kLambdaHi && r0 >= kLambdaLo)) {
            const uint64_t borrow = r0 < kLambdaLo ? 1 : 0;
            r0 -= kLambdaLo;
            r1 = r1 - kLambdaHi - borrow;
            q0 |= 1;
        }
    }
    Glv g;
    g.k1[0] = r0;
    g.k1[1] = r1;
    g.k2[0] = q0;
    g.k2[1] = q1;
    return g;
}

// fr30_mul with a scheduling barrier behind it: these kernels run one workgroup of 64 lanes with every register to spend, and the
// scheduler otherwise interleaves all the independent products it finds, whose operands then no longer fit the register file
__device__ __forceinline__ Fr30 cvb_mul(const Fr30& a, const Fr30& b) {
    const Fr30 r = fr30_mul(a, b);
    __builtin_amdgcn_sched_barrier(0);
    return r;
}
// a blst_fr image at p (32 bytes, 32-byte aligned) into the multiplier form: one product with 2^284
__device__ __forceinline__ Fr30 cvb_ld_m(const uint32_t* __restrict__ p, const Fr30& k284) {
    return cvb_mul(fr30_load(p), k284);
}
__device__ __forceinline__ Fr30 cvb_neg(const Fr30& a) {
    Fr30 r;
#pragma unroll
    for (int i = 0; i < kR9; i++) r.d[i] = -a.d[i];
    return r;
}
// the plain integer of a multiplier-form value, canonical
__device__ __forceinline__ void cvb_plain(const Fr30& a, uint32_t l[8]) { fr30_to_limbs(cvb_mul(a, fr30_small(1)), l); }
__device__ __forceinline__ bool cvb_is_zero(const Fr30& a) { return fr30_is_zero(cvb_mul(a, fr30_small(1))); }
__device__ __forceinline__ void cvb_store_plain(uint32_t* __restrict__ p, const Fr30& a) { fr30_store(p, cvb_mul(a, fr30_small(1))); }
__device__ __forceinline__ void cvb_store_glv(Glv* __restrict__ dst, const Glv& g) {
    uint4* q = reinterpret_cast<uint4*>(dst);
    q[0] = make_uint4((uint32_t)g.k1[0], (uint32_t)(g.k1[0] >> 32), (uint32_t)g.k1[1], (uint32_t)(g.k1[1] >> 32));
    q[1] = make_uint4((uint32_t)g.k2[0], (uint32_t)(g.k2[0] >> 32), (uint32_t)g.k2[1], (uint32_t)(g.k2[1] >> 32));
}
// the split of a multiplier-form value
__device__ __forceinline__ void cvb_emit_glv(Glv* dst, const Fr30* a) {
    uint32_t l[8];
    cvb_plain(*a, l);
    cvb_store_glv(dst, glv_split_device(l));
}

// digit planes of 64 values in LDS
using CvbPlane = Fr30Plane<kCvbThreads>;
// 1 / d for the nonzero d (multiplier form) of each of the workgroup's 64 lanes, which all call: inclusive product scans from
// both ends (six steps of two products), lane 0 inverts the product of all 64 -- ONE fr30_inv -- and lane t takes
// inv x (the lanes before it) x (the lanes after it).  Ends with a barrier, so that the planes can be used again.
__device__ __forceinline__ Fr30 cvb_group_inverse(const Fr30& d, CvbPlane (&pre)[2], CvbPlane (&suf)[2], int32_t (&inv_s)[kR9],
                                                  uint32_t t) {
    Fr30 mp = d, ms = d;
    uint32_t cur = 0;
#pragma unroll 1
    for (uint32_t o = 1; o < kCvbThreads; o <<= 1) {
        plane_put(pre[cur], t, mp);
        plane_put(suf[cur], t, ms);
        __syncthreads();
        if (t >= o) mp = cvb_mul(plane_get(pre[cur], t - o), mp);
        if (t + o < kCvbThreads) ms = cvb_mul(ms, plane_get(suf[cur], t + o));
        cur ^= 1;
    }
    plane_put(pre[cur], t, mp);
    plane_put(suf[cur], t, ms);
    if (t == 0) {  // ms of lane 0 is the product of all
        const Fr30 inv = fr30_inv(ms);
#pragma unroll
        for (int k = 0; k < kR9; k++) inv_s[k] = inv.d[k];
    }
    __syncthreads();
    Fr30 inv;
#pragma unroll
    for (int k = 0; k < kR9; k++) inv.d[k] = inv_s[k];
    if (t > 0) inv = cvb_mul(inv, plane_get(pre[cur], t - 1));
    if (t + 1 < kCvbThreads) inv = cvb_mul(inv, plane_get(suf[cur], t + 1));
    __syncthreads();
    return inv;
}

}  // namespace

// workgroup k < count: out[k] = PI(zeta_k) in multiplier form.  pub: proof k's n_public images at pub + 8 k stride; chal: proof
// k's five challenge images at chal + 40 k, zeta the fourth
__global__ void __launch_bounds__(kCvbThreads) k_cvb_public(const uint32_t* __restrict__ pub, uint32_t n_public, uint64_t stride,
                                                            const uint32_t* __restrict__ chal, const Fr30* __restrict__ consts,
                                                            uint32_t lg_n, Fr30* __restrict__ out) {
    __shared__ CvbPlane pre[2], suf[2];
    __shared__ int32_t inv_s[kR9];
    __shared__ uint32_t hit_s;
    const uint32_t t = threadIdx.x, k = blockIdx.x;
    const Fr30 k284 = fr30_table(consts, kCvbK284), one = fr30_const_one270();
    const Fr30 z = cvb_ld_m(chal + 8 * ((size_t)5 * k + 3), k284);
    const uint32_t* f = pub + 8 * (size_t)k * stride;
    if (t == 0) hit_s = 0xffffffffu;
    Fr30 wcur = one;  // w^t by the six bits of t
    {
        Fr30 base = fr30_table(consts, kCvbW);
#pragma unroll 1
        for (uint32_t bit = 0; bit < 6; bit++) {
            if ((t >> bit) & 1) wcur = cvb_mul(wcur, base);
            base = cvb_mul(base, base);
        }
    }
    const Fr30 w64 = fr30_table(consts, kCvbW64);
    __syncthreads();
    Fr30 acc = fr30_zero();
#pragma unroll 1
    for (uint32_t base = 0; base < n_public; base += kCvbThreads) {
        const uint32_t i = base + t;
        bool live = i < n_public;
        Fr30 d = one;
        if (live) {
            d = cvb_mul(fr30_sub(z, wcur), one);
            if (cvb_is_zero(d)) {
                atomicMin(&hit_s, i);
                d = one;
                live = false;
            }
        }
        const Fr30 dinv = cvb_group_inverse(d, pre, suf, inv_s, t);
        if (live) acc = cvb_mul(fr30_add(acc, cvb_mul(cvb_mul(cvb_ld_m(f + 8 * (size_t)i, k284), wcur), dinv)), one);
        wcur = cvb_mul(wcur, w64);
    }
    // the 64 lanes' sums through LDS (cvb_group_inverse ended with a barrier; without public rounds nothing used the planes)
    plane_put(pre[0], t, acc);
    __syncthreads();
    if (t != 0) return;
    if (hit_s != 0xffffffffu) {
        const Fr30 v = cvb_ld_m(f + 8 * (size_t)hit_s, k284);
#pragma unroll
        for (int q = 0; q < kR9; q++) out[k].d[q] = v.d[q];
        return;
    }
#pragma unroll 1
    for (uint32_t q = 1; q < kCvbThreads; q++) acc = fr30_add(acc, plane_get(pre[0], q));
    Fr30 zn = z;
#pragma unroll 1
    for (uint32_t q = 0; q < lg_n; q++) zn = cvb_mul(zn, zn);
    const Fr30 v = cvb_mul(cvb_mul(acc, one), cvb_mul(fr30_sub(zn, one), fr30_table(consts, kCvbInvN)));
#pragma unroll
    for (int q = 0; q < kR9; q++) out[k].d[q] = v.d[q];
}

// lane k < count.  chal: 5 images per proof (beta, gamma, alpha, zeta, v); evals: 2 t images per proof (abar, sbar, z(zeta w));
// pim: PI(zeta_k) in multiplier form, or null (zero).  lin[4 k ..] (multiplier form): zeta^n, the scalar of [z] in r, the scalar of
// sigma_(t-1), the constant of r
__global__ void __launch_bounds__(kCvbThreads) k_cvb_lin(const uint32_t* __restrict__ chal, const uint32_t* __restrict__ evals,
                                                         const Fr30* __restrict__ pim, const Fr30* __restrict__ consts, uint32_t count,
                                                         uint32_t t, uint32_t lg_n, Fr30* __restrict__ lin) {
    __shared__ CvbPlane pre[2], suf[2];
    __shared__ int32_t inv_s[kR9];
    const uint32_t lane = threadIdx.x, k = blockIdx.x * kCvbThreads + lane;
    const bool active = k < count;
    const Fr30 k284 = fr30_table(consts, kCvbK284), one = fr30_const_one270();
    const uint32_t* ch = chal + 8 * (size_t)5 * (active ? k : 0);
    const uint32_t* ev = evals + 8 * (size_t)2 * t * (active ? k : 0);
    const Fr30 ze = cvb_ld_m(ch + 24, k284);
    Fr30 zn = ze;
#pragma unroll 1
    for (uint32_t q = 0; q < lg_n; q++) zn = cvb_mul(zn, zn);
    // L_0(zeta) = Z / (n (zeta - 1)), and 1 at zeta = 1
    Fr30 d = cvb_mul(fr30_sub(ze, one), one);
    const bool is_one = cvb_is_zero(d);
    if (is_one || !active) d = one;
    const Fr30 dinv = cvb_group_inverse(d, pre, suf, inv_s, lane);
    if (!active) return;
    const Fr30 l0 = is_one ? one : cvb_mul(cvb_mul(fr30_sub(zn, one), fr30_table(consts, kCvbInvN)), dinv);
    const Fr30 be = cvb_ld_m(ch, k284), ga = cvb_ld_m(ch + 8, k284), al = cvb_ld_m(ch + 16, k284);
    Fr30 A = one, B = cvb_ld_m(ev + 8 * (2 * t - 1), k284);
#pragma unroll 1
    for (uint32_t j = 0; j < t; j++) {
        const Fr30 ag = fr30_add(cvb_ld_m(ev + 8 * j, k284), ga);
        A = cvb_mul(A, fr30_add(ag, cvb_mul(cvb_mul(be, fr30_table(consts, kCvbShifts + j)), ze)));
        if (j + 1 < t) B = cvb_mul(B, fr30_add(ag, cvb_mul(be, cvb_ld_m(ev + 8 * (t + j), k284))));
    }
    const Fr30 a2l = cvb_mul(cvb_mul(al, al), l0), aB = cvb_mul(al, B);
    const Fr30 sc_z = fr30_add(cvb_mul(al, A), a2l), sc_sig = cvb_neg(cvb_mul(aB, be));
    Fr30 konst = pim ? fr30_table(pim, k) : fr30_zero();
    konst = fr30_sub(fr30_sub(konst, cvb_mul(aB, fr30_add(cvb_ld_m(ev + 8 * (t - 1), k284), ga))), a2l);
    Fr30* out = lin + 4 * (size_t)k;
#pragma unroll
    for (int q = 0; q < kR9; q++) {
        out[0].d[q] = zn.d[q];
        out[1].d[q] = sc_z.d[q];
        out[2].d[q] = sc_sig.d[q];
        out[3].d[q] = konst.d[q];
    }
}

// v^n by n products (n <= 2 t)
__device__ __forceinline__ Fr30 cvb_pow(const Fr30& v, uint32_t n) {
    Fr30 p = fr30_const_one270();
#pragma unroll 1
    for (uint32_t i = 0; i < n; i++) p = cvb_mul(p, v);
    return p;
}

// lane (k, q), k < count, q < Q = (t + e) + 5 + 2 nk, nk = 2 t + 3 + g: one scalar of proof k each, from k_cvb_lin's record, times
// rho_k.  q < t + e: the proof's own products of A_0 (wire q with v^(1 + q), [z] with r's scalar, chunk c with -Z zeta^(c n)), split
// into glv[k (t + e) + q]; then [z]'s second scalar rho v^(2t) into glv[o_e + k]; the four of stage 2 into s2[4 k ..]; then the 2 nk
// terms of the key side as plain integers into the row rows + 8 (k << log_l): for P0 (times -zeta w) and for P1
__global__ void __launch_bounds__(kCvbThreads) k_cvb_scalars(const uint32_t* __restrict__ chal, const uint32_t* __restrict__ evals,
                                                             const uint32_t* __restrict__ rho, const Fr30* __restrict__ lin,
                                                             const Fr30* __restrict__ consts, const uint8_t* __restrict__ exps,
                                                             uint32_t count, uint32_t t, uint32_t e, uint32_t g,
                                                             Glv* __restrict__ glv, uint64_t o_e, Glv* __restrict__ s2,
                                                             uint32_t* __restrict__ rows, uint32_t log_l) {
    const uint32_t nkey = 2 * t + 2 + g, nk = nkey + 1, per = t + e, Q = per + 5 + 2 * nk;
    const uint64_t id = (uint64_t)blockIdx.x * kCvbThreads + threadIdx.x;
    const uint32_t k = (uint32_t)(id / Q), q = (uint32_t)(id % Q);
    if (k >= count) return;
    const Fr30 k284 = fr30_table(consts, kCvbK284), one = fr30_const_one270();
    const uint32_t* ch = chal + 8 * (size_t)5 * k;
    const uint32_t* ev = evals + 8 * (size_t)2 * t * k;
    const Fr30 r = cvb_ld_m(rho + 8 * (size_t)k, k284);
    Fr30 val = one;     // the value that leaves, without rho
    Fr30 scale = r;     // rho, or rho (-zeta w) for the key side of P0
    Glv* gd = nullptr;  // where it goes: a split scalar, or a plain integer of the row
    uint32_t* rd = nullptr;
    if (q < t) {
        val = cvb_pow(cvb_ld_m(ch + 32, k284), q + 1);
        gd = glv + (size_t)k * per + q;
    } else if (q == t) {
        val = fr30_table(lin, 4 * k + 1);
        gd = glv + (size_t)k * per + q;
    } else if (q < per) {  // chunk c = q - t - 1: -Z zeta^(c n)
        const Fr30 zn = fr30_table(lin, 4 * k);
        val = cvb_mul(cvb_neg(fr30_sub(zn, one)), cvb_pow(zn, q - t - 1));
        gd = glv + (size_t)k * per + q;
    } else if (q == per) {
        val = cvb_pow(cvb_ld_m(ch + 32, k284), 2 * t);
        gd = glv + o_e + k;
    } else if (q < per + 5) {  // the second stage: -zeta w, -zeta, -zeta^2 w on D, E, F for P0 and zeta (1 + w) on F for P1; no rho
        const uint32_t j = q - per - 1;
        const Fr30 ze = cvb_ld_m(ch + 24, k284);
        const Fr30 mzw = cvb_neg(cvb_mul(ze, fr30_table(consts, kCvbW)));
        val = j == 0 ? mzw : (j == 1 ? cvb_neg(ze) : (j == 2 ? cvb_mul(mzw, ze) : cvb_mul(ze, fr30_table(consts, kCvbW1))));
        scale = one;
        gd = s2 + 4 * (size_t)k + j;
    } else {  // the key side: A_0k's coefficient of key commitment j; G1 (j = nkey) also takes A_1k's constant
        const uint32_t jj = q - per - 5, j = jj < nk ? jj : jj - nk;
        const bool p0 = jj < nk;
        rd = rows + 8 * (((size_t)k << log_l) + jj);
        const Fr30 ze = cvb_ld_m(ch + 24, k284);
        const Fr30 mzw = cvb_neg(cvb_mul(ze, fr30_table(consts, kCvbW)));
        if (p0) scale = cvb_mul(r, mzw);
        if (j < t) {
            val = cvb_ld_m(ev + 8 * j, k284);
        } else if (j == t) {
            val = cvb_mul(cvb_ld_m(ev, k284), cvb_ld_m(ev + 8, k284));
        } else if (j == t + 1) {
            val = one;
        } else if (j < 2 * t + 1) {  // sigma_i, i = j - t - 2, with v^(1 + t + i)
            val = cvb_pow(cvb_ld_m(ch + 32, k284), j - 1);
        } else if (j == 2 * t + 1) {
            val = fr30_table(lin, 4 * k + 2);
        } else if (j < nkey) {  // the custom selector s = j - 2 t - 2 with prod_i abar_i^p[s][i]
            const uint32_t sx = j - 2 * t - 2;
            val = one;
#pragma unroll 1
            for (uint32_t i = 0; i < t; i++) {
                const Fr30 a = cvb_ld_m(ev + 8 * i, k284);
#pragma unroll 1
                for (uint32_t c = 0; c < exps[sx * t + i]; c++) val = cvb_mul(val, a);
            }
        } else {  // G1: g0 = the constant of r - sum_(0 < i < 2t) v^i y_i with A_0k's factor, g1 = -v^(2t) z(zeta w) with A_1k's (-zeta)
            const Fr30 v = cvb_ld_m(ch + 32, k284);
            Fr30 g0 = fr30_table(lin, 4 * k + 3), vp = one;
#pragma unroll 1
            for (uint32_t i = 1; i < 2 * t; i++) {
                vp = cvb_mul(vp, v);
                g0 = fr30_sub(g0, cvb_mul(vp, cvb_ld_m(ev + 8 * (i - 1), k284)));
            }
            const Fr30 g1 = cvb_neg(cvb_mul(cvb_mul(vp, v), cvb_ld_m(ev + 8 * (2 * t - 1), k284)));
            if (p0) {  // rho (-zeta w g0 - zeta g1)
                val = fr30_add(cvb_mul(mzw, g0), cvb_mul(cvb_neg(ze), g1));
                scale = r;
            } else {
                val = fr30_add(g0, g1);
            }
        }
    }
    val = cvb_mul(scale, val);
    if (gd) cvb_emit_glv(gd, &val);
    else cvb_store_plain(rd, val);
}

// lane j < n: out[j] = the split of the plain canonical integer sums[j]
__global__ void __launch_bounds__(kCvbThreads) k_cvb_key_split(const uint32_t* __restrict__ sums, uint32_t n, Glv* __restrict__ out) {
    const uint32_t j = blockIdx.x * kCvbThreads + threadIdx.x;
    if (j >= n) return;
    const uint4* q = reinterpret_cast<const uint4*>(sums + 8 * (size_t)j);
    const uint4 a = q[0], b = q[1];
    const uint32_t l[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    cvb_store_glv(out + j, glv_split_device(l));
}

// lane (k, j) = (lane >> 2, lane & 3), k < count.  D, E, F: count XYZZ records each; s: 4 count split scalars, record 4 k + j;
// p0: 3 count records (proof k's terms at 3 k ..), p1: count records
__global__ void __launch_bounds__(kCvbThreads) k_cvb_stage2(const uint4* __restrict__ D, const uint4* __restrict__ E,
                                                            const uint4* __restrict__ F, const Glv* __restrict__ s, uint32_t count,
                                                            uint4* __restrict__ p0, uint4* __restrict__ p1) {
    const uint32_t lane = blockIdx.x * kCvbThreads + threadIdx.x;
    const uint32_t k = lane >> 2, j = lane & 3;
    if (k >= count) return;
    const uint4* src = j == 0 ? D : (j == 1 ? E : F);
    const XYZZ30 y = g1_mul_glv(load_xyzz30(src + (size_t)k * kXyzzU4), load_glv(s, lane));
    uint4* dst = j < 3 ? p0 + ((size_t)3 * k + j) * kXyzzU4 : p1 + (size_t)k * kXyzzU4;
    store_xyzz30(dst, y);
}

void launch_cvb_stage2(hipStream_t st, const void* d_D, const void* d_E, const void* d_F, const Glv* d_s, uint32_t count, void* d_p0,
                       void* d_p1) {
    if (!count) return;
    const uint64_t lanes = (uint64_t)count * 4;
    hipLaunchKernelGGL(k_cvb_stage2, dim3((unsigned)((lanes + kCvbThreads - 1) / kCvbThreads)), dim3(kCvbThreads), 0, st,
                       (const uint4*)d_D, (const uint4*)d_E, (const uint4*)d_F, d_s, count, (uint4*)d_p0, (uint4*)d_p1);
}

void launch_cvb_public(hipStream_t st, const uint32_t* d_pub, uint32_t n_public, uint64_t stride, const uint32_t* d_chal,
                       const Fr30* d_consts, uint32_t lg_n, uint32_t count, Fr30* d_out) {
    if (!count) return;
    hipLaunchKernelGGL(k_cvb_public, dim3(count), dim3(kCvbThreads), 0, st, d_pub, n_public, stride, d_chal, d_consts, lg_n, d_out);
}

void launch_cvb_scalars(hipStream_t st, const uint32_t* d_chal, const uint32_t* d_evals, const uint32_t* d_rho, const Fr30* d_pim,
                        const Fr30* d_consts, const uint8_t* d_exps, uint32_t count, uint32_t t, uint32_t e, uint32_t g, uint32_t lg_n,
                        Fr30* d_lin, Glv* d_glv, uint64_t o_e, Glv* d_s2, uint32_t* d_rows, uint32_t log_l) {
    if (!count) return;
    hipLaunchKernelGGL(k_cvb_lin, dim3((count + kCvbThreads - 1) / kCvbThreads), dim3(kCvbThreads), 0, st, d_chal, d_evals, d_pim,
                       d_consts, count, t, lg_n, d_lin);
    const uint64_t lanes = (uint64_t)count * ((t + e) + 5 + 2 * (2 * t + 3 + g));
    hipLaunchKernelGGL(k_cvb_scalars, dim3((unsigned)((lanes + kCvbThreads - 1) / kCvbThreads)), dim3(kCvbThreads), 0, st, d_chal, d_evals,
                       d_rho, d_lin, d_consts, d_exps, count, t, e, g, d_glv, o_e, d_s2, d_rows, log_l);
}

void launch_cvb_key_split(hipStream_t st, const uint32_t* d_sums, uint32_t n, Glv* d_out) {
    if (!n) return;
    hipLaunchKernelGGL(k_cvb_key_split, dim3((n + kCvbThreads - 1) / kCvbThreads), dim3(kCvbThreads), 0, st, d_sums, n, d_out);
}

}  // namespace kzg
