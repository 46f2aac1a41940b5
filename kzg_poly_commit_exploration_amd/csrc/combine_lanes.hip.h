// combine_lanes.hip.h -- what the streaming sums over 256-lane tiles share (combine_kernels.hip: k_combine_eval, k_sets_combine,
// k_combine_eval_finish; linearise_kernels.hip: k_lin_combine, k_lin_finish): the workgroup sum of 256 lane values and the sum over a polynomial's
// tile records.  Table and coefficient loads and the canonical store are fr30_lanes.hip.h's, which every Fr kernel unit shares.
// Device code only; every function is inlined.
#pragma once
#include <hip/hip_runtime.h>

#include "engine.h"
#include "fr30.hip.h"
#include "fr30_lanes.hip.h"

namespace kzg {

// the digits of another lane of the row (DPP control CTRL) or of the wave (xor MASK) added to this lane's, one carry pass
// each: both operands are carry-normalised, so the raw sum stays within 2^30 + 8 and the top digit only grows (below
// kR9SumTopBound for the 256 products of a workgroup)
template <int CTRL>
__device__ __forceinline__ Fr30 cmb_add_dpp(const Fr30& v) {
    Fr30 o;
#pragma unroll
    for (int k = 0; k < kR9; k++) o.d[k] = __builtin_amdgcn_update_dpp(0, v.d[k], CTRL, 0xf, 0xf, false);
    return fr30_add(v, o);
}
template <int MASK>
__device__ __forceinline__ Fr30 cmb_add_xor(const Fr30& v) {
    Fr30 o;
#pragma unroll
    for (int k = 0; k < kR9; k++) o.d[k] = __shfl_xor(v.d[k], MASK, 64);
    return fr30_add(v, o);
}
// the sum of the workgroup's 256 values (each a product, or a carry-normalised value of that size), carry-normalised, in
// every lane of wave 0; lds: kR9 * 4 words that nothing else touches between two calls
__device__ __forceinline__ Fr30 cmb_workgroup_sum(Fr30 v, int32_t (*lds)[4]) {
    v = cmb_add_dpp<0xb1>(v);   // quad_perm [1, 0, 3, 2]: lane ^ 1
    v = cmb_add_dpp<0x4e>(v);   // quad_perm [2, 3, 0, 1]: lane ^ 2
    v = cmb_add_dpp<0x141>(v);  // row_half_mirror: the other quad of the eight
    v = cmb_add_dpp<0x140>(v);  // row_mirror: the other half of the row
    v = cmb_add_xor<16>(v);
    v = cmb_add_xor<32>(v);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();  // (the previous call's readers are done)
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kR9; k++) lds[k][wave] = v.d[k];
    }
    __syncthreads();
    Fr30 total;
#pragma unroll
    for (int k = 0; k < kR9; k++) total.d[k] = lds[k][0];
#pragma unroll
    for (int w = 1; w < 4; w++) {
        Fr30 o;
#pragma unroll
        for (int k = 0; k < kR9; k++) o.d[k] = lds[k][w];
        total = fr30_add(total, o);
    }
    return total;
}
static_assert(kCombineThreads == 256, "cmb_workgroup_sum adds four wave totals");

// sum_tile rec[tile] W^tile over the `tiles` records at rec (kCombinePartialWords words each), W = z^2048, carry-normalised, in
// every lane of wave 0: lane l takes the tiles l + 256 m by Horner in W^256, times W^l, then the workgroup sum.  A record is a
// carry-normalised sum of 256 products (below 128.1 r, top digit below 2^22): with a product added raw it is still an operand
// fr30_mul takes, and every product comes back below 0.51 r, so the workgroup's sum obeys the bound of the tile kernels'.
__device__ __forceinline__ Fr30 cmb_tiles_sum(const uint32_t* __restrict__ rec, uint32_t tiles, const Fr30* __restrict__ tab,
                                              int32_t (*lds)[4]) {
    const uint32_t l = threadIdx.x;
    const Fr30 w256 = fr30_table(tab, kCombineTabW256);
    Fr30 h = fr30_zero();
    if (l < tiles) {
        const uint32_t top = (tiles - 1 - l) / kCombineThreads;  // the lane's tiles are l + 256 m, m <= top
#pragma unroll 1
        for (uint32_t m = top + 1; m-- > 0;) {
            const uint4* q = reinterpret_cast<const uint4*>(rec + ((size_t)l + (size_t)m * kCombineThreads) * kCombinePartialWords);
            const uint4 a = q[0], b = q[1], c = q[2];
            Fr30 v;
            v.d[0] = (int32_t)a.x; v.d[1] = (int32_t)a.y; v.d[2] = (int32_t)a.z; v.d[3] = (int32_t)a.w;
            v.d[4] = (int32_t)b.x; v.d[5] = (int32_t)b.y; v.d[6] = (int32_t)b.z; v.d[7] = (int32_t)b.w;
            v.d[8] = (int32_t)c.x;
            h = fr30_add_raw(fr30_mul(h, w256), v);
        }
        h = fr30_mul(h, fr30_mul(fr30_table(tab, kCombineTabWa + (l >> 4)), fr30_table(tab, kCombineTabWb + (l & 15))));
    }
    return cmb_workgroup_sum(h, lds);
}

}  // namespace kzg
