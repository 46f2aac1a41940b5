// blind_kernels.hip -- zero-knowledge blinding of a circuit proof's polynomials (kzg_blind_evaluations, kzg_circuit_quotient_blinded,
// kzg_circuit_open_blinded).
//
// A blinded column is f~(X) = f(X) + b(X) (X^n - 1) with deg b < nb <= 3: it agrees with f on H, and in coefficient form the
// blinder is a patch of at most 2 nb coefficients -- minus b at 0 .. nb - 1, plus b at n .. n + nb - 1.
//   k_blind_patch  one workgroup of 64 lanes per column.  At n < nb the two index ranges overlap (index n + i is also an index
//                  i' < nb), so every touched index has ONE owning lane, which forms it once from the column's old value, the low
//                  blinder and the high blinder: there is no order of writes to get wrong.  All lanes zero the padding
//                  [n + nb, stride).  The low and the high blinders are given apart, so that the chunks of
//                  the quotient (T~_c = T_c + d_c X^n - d_(c-1)) go through the same kernel; columns from k_hi on only lose their
//                  low blinder: their entries from n on (the last chunk's own coefficients) are left alone.
//   k_blind_tail   the last round's sums past index n.  k_lin_combine (linearise_kernels.hip) has summed the columns over [0, n)
//                  from their UNBLINDED coefficients, the resident key's among them, which end at n and are never read past it.
//                  This kernel adds what the blinders change: for every per-proof column a record (multiplier, tail, low) says
//                  what the column holds at n + i (its high blinder, or for T's last chunk its own coefficients on the device)
//                  and what is taken off at i < 3.  One workgroup; lane j < ntail owns index n + j, lanes ntail .. ntail + 2 the
//                  indices 0 .. 2 below n.  A lane forms  out[idx] = (idx < n ? out[idx] : 0) + sum_k mult_k (tail_k[idx - n] -
//                  low_k[idx])  and the change of out(z):  y += sum_idx delta[idx] z^idx,  with the powers z^idx from the host.
//
// Forms (fr30.hip.h): coefficients, blinders, out and y are blst_fr images (x 2^256); the multipliers and the powers of z carry
// 2^270 (fr30_arg_from_mont256), so a product of a value and a multiplier is a value.
#include <hip/hip_runtime.h>

#include "combine_lanes.hip.h"
#include "engine.h"
#include "fr30.hip.h"

namespace kzg {

namespace {

constexpr uint32_t kPatchThreads = 64;

// cols: k columns, column c at cols + 8 c stride words, n coefficients each (canonical).  lo, hi: nb canonical values per column
// (column c at + 8 c nb words).  Column c < k_hi becomes  f - lo (X^0 ..) + hi X^n  with zeros up to the stride; a column from
// k_hi on only loses lo.  Every touched value is a canonical value plus and minus one canonical value: inside (-r, 2r), which
// fr30_to_limbs canonicalises.  stride >= n + nb for the columns below k_hi.
__global__ void __launch_bounds__(kPatchThreads) k_blind_patch(uint32_t* cols, uint32_t n, uint64_t stride, const uint32_t* __restrict__ lo,
                                                               const uint32_t* __restrict__ hi, uint32_t nb, uint32_t k_hi) {
    const uint32_t c = blockIdx.x, l = threadIdx.x;
    uint32_t* col = cols + 8 * (uint64_t)c * stride;
    const bool high = c < k_hi;
    const uint32_t* blo = lo + 8 * (uint64_t)c * nb;
    const uint32_t* bhi = hi + 8 * (uint64_t)c * nb;
    // every touched index has ONE owner, which forms it from the column's old value and the two blinders: lane i < nb owns index
    // i where that is below n, lane nb + i owns index n + i (which at n < nb is also a low index: it loses blo[n + i] there)
    if (l < nb && l < n) {
        fr30_store(col + 8 * (uint64_t)l, fr30_sub(fr30_load(col + 8 * (uint64_t)l), fr30_load(blo + 8 * l)));
    } else if (high && l >= nb && l < 2 * nb) {
        const uint64_t idx = (uint64_t)n + (l - nb);
        Fr30 v = fr30_load(bhi + 8 * (l - nb));
        if (idx < nb) v = fr30_sub(v, fr30_load(blo + 8 * idx));
        fr30_store(col + 8 * idx, v);
    }
    if (high) {
        for (uint64_t idx = (uint64_t)n + nb + l; idx < stride; idx += kPatchThreads) {
            uint4* q = reinterpret_cast<uint4*>(col + 8 * idx);
            q[0] = make_uint4(0u, 0u, 0u, 0u);
            q[1] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
}

// cols: ncols <= kBlindMaxColumns records.  out: n + ntail values, [0, n) written by k_lin_combine; y: out(z) over [0, n), as
// k_lin_finish left it.  pw: ntail + kBlindLow multipliers, pw[j] = z^(n + j) for j < ntail, pw[ntail + i] = z^i.
// Bound (fr30.hip.h, fr30_mac): an accumulator starts as zero or as one canonical value and takes at most 2 kBlindMaxColumns = 32
// products v * mult / 2^270 with v < 2^256 and the multiplier canonical: each below 0.5001 r + r / 2^14, the sum below 17.1 r --
// inside the 256 products fr30_mac documents, as in k_lin_combine.  fr30_sum_reduce brings it under 0.51 r before it leaves.
__global__ void __launch_bounds__(kCombineThreads) k_blind_tail(const BlindColumn* __restrict__ cols, uint32_t ncols, uint32_t n,
                                                                uint32_t ntail, const Fr30* __restrict__ pw, uint32_t* out,
                                                                uint32_t* y) {
    __shared__ int32_t lds[kR9][4];
    const uint32_t l = threadIdx.x;
    // the lane's index: n + l, or a low index below n (a low index >= n is some lane's n + j already: ntail >= kBlindLow)
    const bool is_tail = l < ntail;
    const uint32_t low_i = l - ntail;
    const bool is_low = !is_tail && low_i < kBlindLow && low_i < n;
    const uint64_t idx = is_tail ? (uint64_t)n + l : low_i;
    Fr30 delta = fr30_zero();
    if (is_tail || is_low) {
#pragma unroll 1
        for (uint32_t k = 0; k < ncols; k++) {
            Fr30 w, neg;
#pragma unroll
            for (int d = 0; d < kR9; d++) {
                w.d[d] = cols[k].mult[d];
                neg.d[d] = -w.d[d];
            }
            if (is_tail && l < cols[k].tail_len) delta = fr30_mac(delta, fr30_load(cols[k].tail + 8 * (uint64_t)l), w);
            if (idx < kBlindLow && cols[k].low) delta = fr30_mac(delta, fr30_load(cols[k].low + 8 * idx), neg);
        }
        delta = fr30_sum_reduce(delta);
        Fr30 v = delta;
        if (idx < n) v = fr30_add(v, fr30_load(out + 8 * idx));  // |v| < 0.51 r + r: inside (-r, 2r)
        fr30_store(out + 8 * idx, v);
        delta = fr30_mul(delta, fr30_table(pw, is_tail ? l : ntail + low_i));
    }
    const Fr30 total = cmb_workgroup_sum(delta, lds);
    if (l == 0) fr30_store(y, fr30_sum_reduce(fr30_add(total, fr30_load(y))));
}

}  // namespace

void launch_blind_patch(hipStream_t s, uint32_t* d_cols, uint32_t n, uint64_t k, uint64_t stride, const uint32_t* d_lo,
                        const uint32_t* d_hi, uint32_t nb, uint64_t k_hi) {
    if (!k || !nb) return;
    hipLaunchKernelGGL(k_blind_patch, dim3((unsigned)k), dim3(kPatchThreads), 0, s, d_cols, n, stride, d_lo, d_hi, nb, (uint32_t)k_hi);
}

void launch_blind_tail(hipStream_t s, const BlindColumn* d_cols, uint32_t ncols, uint32_t n, uint32_t ntail, const Fr30* d_pw,
                       uint32_t* d_out, uint32_t* d_y) {
    if (ncols > kBlindMaxColumns || ntail < kBlindLow || ntail + kBlindLow > kCombineThreads) return;
    hipLaunchKernelGGL(k_blind_tail, dim3(1), dim3(kCombineThreads), 0, s, d_cols, ncols, n, ntail, d_pw, d_out, d_y);
}

}  // namespace kzg
