// combine_kernels.hip -- many polynomials, one point, one proof (kzg_open_combined).
//
//     F = sum_{i < t} gamma^i P_i,        y_i = P_i(z),        proof = [q(s)]G1 with q = (F - F(z)) / (X - z)
//
// The quotient and the MSM are the ones of a single opening, run on F; what is new is the pass that makes F and the t
// values while every coefficient is read ONCE:
//   k_combine_eval         grid = tiles of kCombineTile = 2048 consecutive indices, 256 lanes.  Lane l owns the indices
//                          l + 256 m (m < 8) of the tile for ALL polynomials of the pass: consecutive lanes read consecutive
//                          32-byte coefficients, nothing is staged in LDS.  Per polynomial i the lane adds c * gamma^i to its
//                          eight accumulators (fr30_mac; the multiplier gamma^i * 2^270 is read uniformly from the table the
//                          host prepared) and forms sum_m c_m (z^256)^m by Horner, times z^l (computed once per lane from a
//                          16 + 16 entry table, reused for every polynomial).  The 256 lane values are summed -- four DPP
//                          steps inside a row of 16 lanes, two shuffles across the rows of a wave, one exchange of the four
//                          wave totals through LDS -- into one 12-word digit record per (polynomial, tile).  After the last
//                          polynomial the accumulators (plus F of the earlier passes, carried canonically) leave as canonical
//                          blst_fr.
//   k_combine_eval_finish  one workgroup per polynomial: y_i = sum_tiles e_(i,tile) (z^2048)^tile, the same lane pattern one
//                          level up (lane l takes the tiles l + 256 m, Horner in W^256, times W^l, W = z^2048), canonical out.
//
// Forms (fr30.hip.h): coefficients, F and the y_i are blst_fr images (x 2^256); gamma^i and every power of z carry 2^270,
// so a product of a value and a multiplier is a value, of two multipliers a multiplier.
#include <hip/hip_runtime.h>

#include "combine_lanes.hip.h"
#include "engine.h"
#include "fr30.hip.h"

namespace kzg {

namespace {

constexpr uint32_t kCombineRun = kCombineTile / kCombineThreads;  // indices per lane: 8
constexpr int RUN = (int)kCombineRun;

// The walks over a lane's eight indices, unrolled by recursion over the index (the compiler leaves a loop of sixteen
// products rolled, and the accumulators it then indexes would live in scratch).
// index M, from the top: acc[M] += c * g, h = h z^256 + c (Horner: the raw sum of a product and a coefficient is an operand
// fr30_mul takes as it is); a coefficient past n counts as zero
template <int M>
__device__ __forceinline__ void cmb_steps(Fr30 (&acc)[kCombineRun], Fr30& h, const uint4 (&lo)[kCombineRun],
                                          const uint4 (&hi)[kCombineRun], const Fr30& g, const Fr30& z256, uint64_t base,
                                          uint32_t n) {
    Fr30 c = fr30_from_u4(lo[M], hi[M]);
    if (base + (uint64_t)M * kCombineThreads >= n) c = fr30_zero();
    acc[M] = fr30_mac(acc[M], c, g);
    h = fr30_add_raw(fr30_mul(h, z256), c);
    if constexpr (M > 0) cmb_steps<M - 1>(acc, h, lo, hi, g, z256, base, n);
}
template <int M>
__device__ __forceinline__ void cmb_store_f(const Fr30 (&acc)[kCombineRun], uint32_t* f, uint64_t base, uint32_t n) {
    const uint64_t idx = base + (uint64_t)M * kCombineThreads;
    if (idx < n) fr30_store(f + 8 * idx, fr30_sum_reduce(acc[M]));
    if constexpr (M + 1 < RUN) cmb_store_f<M + 1>(acc, f, base, n);
}

// coeffs: polynomial i (i < t) at coeffs + 8 i stride words, n coefficients each; tab: the host's multipliers
// (CombineTable: powers of z, then gamma^(first + i) at kCombineTabGamma + i for this pass's first polynomial `first`,
// already added to the pointer `gam`); f: F, n canonical values, read first when carry != 0 (the earlier passes' sum) and
// written; partial: record (i, tile) at 12 (i tiles + tile) words.
__global__ void __launch_bounds__(kCombineThreads) k_combine_eval(const uint32_t* __restrict__ coeffs, uint32_t n, uint32_t t,
                                                                  uint64_t stride, const Fr30* __restrict__ tab,
                                                                  const Fr30* __restrict__ gam, int carry, uint32_t* f,
                                                                  uint32_t* __restrict__ partial) {
    __shared__ int32_t lds[kR9][4];
    const uint32_t l = threadIdx.x, tile = blockIdx.x, tiles = gridDim.x;
    const uint64_t base = (uint64_t)tile * kCombineTile + l;  // index of the lane's first coefficient
    // z^l = z^(16 (l >> 4)) z^(l & 15), a multiplier again
    const Fr30 zl = fr30_mul(fr30_table(tab, kCombineTabPa + (l >> 4)), fr30_table(tab, kCombineTabPb + (l & 15)));
    const Fr30 z256 = fr30_table(tab, kCombineTabZ256);
    // The accumulators.  Bound (fr30.hip.h, fr30_mac): each starts as zero or a canonical value and takes at most
    // KZG_MAX_COMBINE = 256 products c * gamma^i / 2^270 with c < 2^256 and the multiplier canonical (< r): every product is
    // below 0.5001 r + r / 2^14 in magnitude, the sum below 129.1 r, its top digit below kR9SumTopBound = 2^22; digits 0..7
    // are carry-normalised after EVERY product, because a raw sum of a normalised value and one product already reaches
    // 2^30 + 4 and fr30_norm takes digits below 2^31 - 2^29 only.  One product with one brings the sum back under 0.51 r
    // (fr30_sum_reduce) before fr30_to_limbs, whose input range is (-r, 2r).
    Fr30 acc[kCombineRun];
#pragma unroll
    for (int m = 0; m < RUN; m++) {
        const uint64_t idx = base + (uint64_t)m * kCombineThreads;
        acc[m] = fr30_zero();
        if (carry && idx < n) {
            const uint4* q = reinterpret_cast<const uint4*>(f) + 2 * idx;
            acc[m] = fr30_from_u4(q[0], q[1]);
        }
    }
#pragma unroll 1
    for (uint32_t i = 0; i < t; i++) {
        const uint4* src = reinterpret_cast<const uint4*>(coeffs) + 2 * ((uint64_t)i * stride);
        // all sixteen loads of the lane are issued before the first product; an index past n reads the polynomial's
        // coefficient 0 instead (n >= 1) and counts as zero
        uint4 lo[kCombineRun], hi[kCombineRun];
#pragma unroll
        for (int m = 0; m < RUN; m++) {
            const uint64_t idx = base + (uint64_t)m * kCombineThreads;
            const uint4* p = src + 2 * (idx < n ? idx : 0);
            lo[m] = p[0];
            hi[m] = p[1];
        }
        const Fr30 g = fr30_table(gam, i);
        Fr30 h = fr30_zero();
        cmb_steps<RUN - 1>(acc, h, lo, hi, g, z256, base, n);
        const Fr30 e = cmb_workgroup_sum(fr30_mul(h, zl), lds);
        if (l == 0) {
            uint4* q = reinterpret_cast<uint4*>(partial + ((size_t)i * tiles + tile) * kCombinePartialWords);
            q[0] = make_uint4((uint32_t)e.d[0], (uint32_t)e.d[1], (uint32_t)e.d[2], (uint32_t)e.d[3]);
            q[1] = make_uint4((uint32_t)e.d[4], (uint32_t)e.d[5], (uint32_t)e.d[6], (uint32_t)e.d[7]);
            q[2] = make_uint4((uint32_t)e.d[8], 0u, 0u, 0u);
        }
    }
    cmb_store_f<0>(acc, f, base, n);
}

// out[i] = sum_tile partial[i][tile] W^tile (canonical), W = z^2048.  A record is a carry-normalised sum of 256 products
// (below 128.1 r, top digit below 2^22): with a product added raw it is still an operand fr30_mul takes, and every
// product comes back below 0.51 r, so the workgroup's sum obeys the bound of k_combine_eval's.
__global__ void __launch_bounds__(kCombineThreads) k_combine_eval_finish(const uint32_t* __restrict__ partial, uint32_t tiles,
                                                                         const Fr30* __restrict__ tab,
                                                                         uint32_t* __restrict__ out) {
    __shared__ int32_t lds[kR9][4];
    const uint32_t l = threadIdx.x, i = blockIdx.x;
    const uint32_t* rec = partial + (size_t)i * tiles * kCombinePartialWords;
    const Fr30 y = cmb_tiles_sum(rec, tiles, tab, lds);
    if (l == 0) fr30_store(out + 8 * (size_t)i, fr30_sum_reduce(y));
}

// ---- openings at several point sets (kzg_open_sets) ---------------------------------------------------
// One pass per distinct point p: G_p = sum_j mult_j P_sel[j] and the values P_sel[j](p), every coefficient read once.  It is
// k_combine_eval with a selection list: polynomial j of the pass sits at coeffs + 8 (sel[j] - sel_base) stride words (sel
// holds indices of the call, sel_base the index of the first polynomial resident at coeffs), and its multiplier
// gamma^i w_(g(i),p) x 2^270 -- canonical, prepared by the host -- is mult[j]; tab: the 66 powers of p in k_combine_eval's
// layout.  g: G_p, read first when carry != 0.  The bound above
// fr30_mac holds unchanged: an accumulator starts as zero or a canonical value and takes at most KZG_MAX_COMBINE = 256
// products of a coefficient below 2^256 and a canonical multiplier.
__global__ void __launch_bounds__(kCombineThreads) k_sets_combine(const uint32_t* __restrict__ coeffs, uint32_t n, uint32_t t,
                                                                  uint64_t stride, const Fr30* __restrict__ tab,
                                                                  const Fr30* __restrict__ mult,
                                                                  const uint32_t* __restrict__ sel, uint32_t sel_base, int carry,
                                                                  uint32_t* g, uint32_t* __restrict__ partial) {
    __shared__ int32_t lds[kR9][4];
    const uint32_t l = threadIdx.x, tile = blockIdx.x, tiles = gridDim.x;
    const uint64_t base = (uint64_t)tile * kCombineTile + l;
    const Fr30 zl = fr30_mul(fr30_table(tab, kCombineTabPa + (l >> 4)), fr30_table(tab, kCombineTabPb + (l & 15)));
    const Fr30 z256 = fr30_table(tab, kCombineTabZ256);
    Fr30 acc[kCombineRun];
#pragma unroll
    for (int m = 0; m < RUN; m++) {
        const uint64_t idx = base + (uint64_t)m * kCombineThreads;
        acc[m] = fr30_zero();
        if (carry && idx < n) {
            const uint4* q = reinterpret_cast<const uint4*>(g) + 2 * idx;
            acc[m] = fr30_from_u4(q[0], q[1]);
        }
    }
#pragma unroll 1
    for (uint32_t j = 0; j < t; j++) {
        const uint4* src = reinterpret_cast<const uint4*>(coeffs) + 2 * ((uint64_t)(sel[j] - sel_base) * stride);
        uint4 lo[kCombineRun], hi[kCombineRun];
#pragma unroll
        for (int m = 0; m < RUN; m++) {
            const uint64_t idx = base + (uint64_t)m * kCombineThreads;
            const uint4* p = src + 2 * (idx < n ? idx : 0);
            lo[m] = p[0];
            hi[m] = p[1];
        }
        const Fr30 w = fr30_table(mult, j);
        Fr30 h = fr30_zero();
        cmb_steps<RUN - 1>(acc, h, lo, hi, w, z256, base, n);
        const Fr30 e = cmb_workgroup_sum(fr30_mul(h, zl), lds);
        if (l == 0) {
            uint4* q = reinterpret_cast<uint4*>(partial + ((size_t)j * tiles + tile) * kCombinePartialWords);
            q[0] = make_uint4((uint32_t)e.d[0], (uint32_t)e.d[1], (uint32_t)e.d[2], (uint32_t)e.d[3]);
            q[1] = make_uint4((uint32_t)e.d[4], (uint32_t)e.d[5], (uint32_t)e.d[6], (uint32_t)e.d[7]);
            q[2] = make_uint4((uint32_t)e.d[8], 0u, 0u, 0u);
        }
    }
    cmb_store_f<0>(acc, g, base, n);
}

}  // namespace

void launch_sets_combine(hipStream_t s, const uint32_t* d_coeffs, uint32_t n, uint32_t t, uint64_t stride, const Fr30* d_tab,
                         const Fr30* d_mult, const uint32_t* d_sel, uint32_t sel_base, bool carry, uint32_t* d_g, uint32_t* d_partial,
                         uint32_t* d_ys) {
    if (!n || !t) return;
    const uint32_t tiles = combine_tiles(n);
    hipLaunchKernelGGL(k_sets_combine, dim3(tiles), dim3(kCombineThreads), 0, s, d_coeffs, n, t, stride, d_tab, d_mult, d_sel,
                       sel_base,
                       carry ? 1 : 0, d_g, d_partial);
    hipLaunchKernelGGL(k_combine_eval_finish, dim3(t), dim3(kCombineThreads), 0, s, (const uint32_t*)d_partial, tiles, d_tab,
                       d_ys);
}

void launch_combine_eval(hipStream_t s, const uint32_t* d_coeffs, uint32_t n, uint32_t t, uint64_t stride, const Fr30* d_tab,
                         uint32_t first, bool carry, uint32_t* d_f, uint32_t* d_partial, uint32_t* d_ys) {
    if (!n || !t) return;
    const uint32_t tiles = combine_tiles(n);
    hipLaunchKernelGGL(k_combine_eval, dim3(tiles), dim3(kCombineThreads), 0, s, d_coeffs, n, t, stride, d_tab,
                       d_tab + kCombineTabGamma + first, carry ? 1 : 0, d_f, d_partial);
    hipLaunchKernelGGL(k_combine_eval_finish, dim3(t), dim3(kCombineThreads), 0, s, (const uint32_t*)d_partial, tiles, d_tab,
                       d_ys);
}

}  // namespace kzg
