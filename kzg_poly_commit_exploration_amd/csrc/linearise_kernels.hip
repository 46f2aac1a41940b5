// linearise_kernels.hip -- a weighted sum of columns that live in DIFFERENT buffers, and its value at one point
// (kzg_circuit_open, kzg_circuit_linearise).
//
//     out[i] = sum_{k < ncols} mult_k C_k[i]   (+ konst at i = 0),          y = out(z)
//
// The last round of a circuit's proof opens the linearisation polynomial r together with the wires and the sigmas at zeta.  r is a
// sum of the resident key's columns, z and the chunks of T with scalars the host knows once the evaluations are in, so
// G_zeta = m_0 r + sum m_i P_i is ONE sum over 3 t + e + 2 columns, none of which is copied and r itself is never stored:
//   k_lin_combine  grid = tiles of kCombineTile = 2048 consecutive indices, 256 lanes, lane l owning l + 256 m (m < 8) -- the
//                  geometry and arithmetic of k_sets_combine (combine_kernels.hip).  The lane takes its eight indices in two
//                  halves of four (148 registers instead of 226: the kernel runs beside another slot's accumulation).  Per half
//                  and column it issues its eight loads, reads the column's record (pointer, multiplier) uniformly and adds
//                  c * mult to its four accumulators (fr30_mac).  The column loop is not unrolled.  After the last column the
//                  accumulators leave as canonical blst_fr, and the same values go through Horner in z^256; the lane's sum times
//                  z^l goes through the workgroup sum into one 12-word digit record per tile.
//   k_lin_finish   one workgroup: y = sum_tiles e_tile (z^2048)^tile, as k_combine_eval_finish does it for one polynomial.
//
// Forms (fr30.hip.h): coefficients, konst, out and y are blst_fr images (x 2^256); the multipliers and the powers of z carry
// 2^270 (fr30_arg_from_mont256), so a product of a value and a multiplier is a value.
//
// The lane helpers (cmb_*) are those of combine_kernels.hip, shared through combine_lanes.hip.h.
#include <hip/hip_runtime.h>

#include "combine_lanes.hip.h"
#include "engine.h"
#include "fr30.hip.h"

namespace kzg {

namespace {

constexpr int RUN = (int)(kCombineTile / kCombineThreads);  // indices per lane: 8
constexpr int HALF = RUN / 2;

// The walks over the HALF indices of one half of a lane's run (index m of the half is base + 256 m), unrolled: a rolled loop would
// index the accumulators, which would then live in scratch.
// One column: the eight loads are issued before the first product; an index past n reads the column's coefficient 0 instead
// (n >= 1) and counts as zero.  acc[m] += c * w
__device__ __forceinline__ void lin_column(Fr30 (&acc)[HALF], const uint4* __restrict__ src, const Fr30& w, uint64_t base, uint32_t n) {
    uint4 lo[HALF], hi[HALF];
#pragma unroll
    for (int m = 0; m < HALF; m++) {
        const uint64_t idx = base + (uint64_t)m * kCombineThreads;
        const uint4* p = src + 2 * (idx < n ? idx : 0);
        lo[m] = p[0];
        hi[m] = p[1];
    }
#pragma unroll
    for (int m = 0; m < HALF; m++) {
        Fr30 c = fr30_from_u4(lo[m], hi[m]);
        if (base + (uint64_t)m * kCombineThreads >= n) c = fr30_zero();
        acc[m] = fr30_mac(acc[m], c, w);
    }
}
// index M, from the top: the accumulator comes back under 0.51 r (fr30_sum_reduce), leaves as a canonical value and enters
// h = h z^256 + v (the raw sum of a product and a value of that size is an operand fr30_mul takes)
template <int M>
__device__ __forceinline__ void lin_leave(const Fr30 (&acc)[HALF], Fr30& h, const Fr30& z256, uint32_t* out, uint64_t base,
                                          uint32_t n) {
    const uint64_t idx = base + (uint64_t)M * kCombineThreads;
    const Fr30 v = fr30_sum_reduce(acc[M]);
    if (idx < n) fr30_store(out + 8 * idx, v);
    h = fr30_add_raw(fr30_mul(h, z256), v);
    if constexpr (M > 0) lin_leave<M - 1>(acc, h, z256, out, base, n);
}

// cols: ncols <= kLinMaxColumns records; tab: the 66 powers of z in k_combine_eval's layout; konst: a canonical blst_fr added to
// out[0]; out: n canonical values, written (no column may overlap it); partial: one record of kCombinePartialWords words per tile.
__global__ void __launch_bounds__(kCombineThreads, 3) k_lin_combine(const LinColumn* __restrict__ cols, uint32_t ncols, uint32_t n,
                                                                 const Fr30* __restrict__ tab, LinConst konst, uint32_t* out,
                                                                 uint32_t* __restrict__ partial) {
    __shared__ int32_t lds[kR9][4];
    const uint32_t l = threadIdx.x, tile = blockIdx.x;
    const uint64_t base = (uint64_t)tile * kCombineTile + l;  // index of the lane's first coefficient
    // The accumulators.  Bound (fr30.hip.h, fr30_mac): each starts as zero or as the canonical constant and takes at most
    // kLinMaxColumns = 32 products c * mult / 2^270 with c < 2^256 and the multiplier canonical (< r): every product is below
    // 0.5001 r + r / 2^14 in magnitude, the sum below 17.1 r -- inside the 256 products (129.1 r, top digit below kR9SumTopBound)
    // that fr30_mac documents for k_sets_combine; digits 0..7 are carry-normalised after EVERY product.  One product with one
    // brings the sum back under 0.51 r (fr30_sum_reduce) before fr30_to_limbs, whose input range is (-r, 2r).
    // A lane takes its run in two halves, the upper one first (Horner runs from the top): four accumulators (36 registers) and
    // eight loads in flight instead of eight and sixteen, which is what keeps the kernel inside 160 registers.  Every coefficient
    // is still read once; the table is walked twice.
    const Fr30 z256 = fr30_table(tab, kCombineTabZ256);
    Fr30 h = fr30_zero();
#pragma unroll 1
    for (int half = RUN / HALF - 1; half >= 0; half--) {
        const uint64_t first = base + (uint64_t)half * HALF * kCombineThreads;
        Fr30 acc[HALF];
#pragma unroll
        for (int m = 0; m < HALF; m++) acc[m] = fr30_zero();
        if (first == 0) acc[0] = fr30_from_limbs(konst.l);
#pragma unroll 1
        for (uint32_t k = 0; k < ncols; k++) {
            Fr30 w;
#pragma unroll
            for (int d = 0; d < kR9; d++) w.d[d] = cols[k].mult[d];
            lin_column(acc, reinterpret_cast<const uint4*>(cols[k].coeffs), w, first, n);
        }
        lin_leave<HALF - 1>(acc, h, z256, out, first, n);
    }
    // z^l = z^(16 (l >> 4)) z^(l & 15), a multiplier again
    const Fr30 zl = fr30_mul(fr30_table(tab, kCombineTabPa + (l >> 4)), fr30_table(tab, kCombineTabPb + (l & 15)));
    const Fr30 e = cmb_workgroup_sum(fr30_mul(h, zl), lds);
    if (l == 0) {
        uint4* q = reinterpret_cast<uint4*>(partial + (size_t)tile * kCombinePartialWords);
        q[0] = make_uint4((uint32_t)e.d[0], (uint32_t)e.d[1], (uint32_t)e.d[2], (uint32_t)e.d[3]);
        q[1] = make_uint4((uint32_t)e.d[4], (uint32_t)e.d[5], (uint32_t)e.d[6], (uint32_t)e.d[7]);
        q[2] = make_uint4((uint32_t)e.d[8], 0u, 0u, 0u);
    }
}

// y = sum_tile partial[tile] W^tile (canonical), W = z^2048: k_combine_eval_finish for one polynomial
__global__ void __launch_bounds__(kCombineThreads) k_lin_finish(const uint32_t* __restrict__ partial, uint32_t tiles,
                                                                const Fr30* __restrict__ tab, uint32_t* __restrict__ y) {
    __shared__ int32_t lds[kR9][4];
    const Fr30 total = cmb_tiles_sum(partial, tiles, tab, lds);
    if (threadIdx.x == 0) fr30_store(y, fr30_sum_reduce(total));
}

}  // namespace

void launch_lin_combine(hipStream_t s, const LinColumn* d_cols, uint32_t ncols, uint32_t n, const Fr30* d_tab, const LinConst& konst,
                        uint32_t* d_out, uint32_t* d_partial, uint32_t* d_y) {
    if (!n || !ncols || ncols > kLinMaxColumns) return;
    const uint32_t tiles = combine_tiles(n);
    hipLaunchKernelGGL(k_lin_combine, dim3(tiles), dim3(kCombineThreads), 0, s, d_cols, ncols, n, d_tab, konst, d_out, d_partial);
    hipLaunchKernelGGL(k_lin_finish, dim3(1), dim3(kCombineThreads), 0, s, (const uint32_t*)d_partial, tiles, d_tab, d_y);
}

}  // namespace kzg
