// multilinear_kernels.hip -- opening a multilinear polynomial given by its n = 2^l values on the boolean hypercube
// (Gemini / HyperKZG over the KZG setup).
//
//     f_(i+1)[j] = f_i[2j] + u_i (f_i[2j+1] - f_i[2j]),   j < n >> (i+1),   f_0 = the values, f_l = the one value v = f~(u)
//     y_(i,0) = f_i(r), y_(i,1) = f_i(-r), y_(i,2) = f_i(r^2)   (f_i read as coefficients)
//     F[j] = sum_{i < l, j < n >> i} gamma^i f_i[j]
//
// The pyramid: levels f_1 .. f_l packed in one buffer of n - 1 values, level i at offset n - (n >> (i - 1)).
//
//   k_ml_fold         256 lanes, a tile of 2048 consecutive values of the source level: its slice of the next (up to) eleven
//                     levels needs no other workgroup's data.  Three levels in the lane's registers, six across the wave by
//                     shuffles, two across the four waves through LDS; every level's slice goes to its place in the pyramid.
//                     Two launches fold any l <= 22: the values down to level min(l, 11), then ONE workgroup folds the <= 2048
//                     values of level 11 down to v.  No kernel waits on another workgroup.
//                     Load pattern: a lane reads its eight consecutive values, 256 contiguous bytes, as sixteen 16-byte loads
//                     issued together (64 contiguous bytes per pair it folds).  One load instruction of a wave is strided by 256
//                     bytes, but a lane consumes both 128-byte lines it touches in full with back-to-back loads, so every line
//                     is fetched from HBM once; the lane-contiguous layout is what lets three levels fold with no exchange at
//                     all.  The stores of a level are contiguous over the lanes that hold it.
//   k_ml_eval         grid (tiles of level 0, levels): k_combine_eval's lane pattern (lane t owns the indices t + 256 m, m < 8,
//                     of its tile) with a length and an offset per level.  All indices of a lane have the parity of t, and the
//                     tile base and the stride 256 are even: ONE Horner chain in r^256 = (-r)^256 times r^t is the lane's share
//                     at r, and (-1)^t times it the share at -r (the even and the odd indices are the even and the odd lanes).
//                     A second chain in (r^2)^256 gives the share at r^2.  Three 12-word records per (level, tile).
//   k_ml_eval_finish  one workgroup per (level, point): sums the tiles with the powers of the tile step (cmb_tiles_sum; the
//                     step r^2048 serves r and -r), canonical out.  A level shorter than a tile takes the same path, indices past
//                     its length counting as zero.
//   k_ml_combine      F, one index per lane, at most 22 terms per accumulator, canonical out.
//
// Forms (fr30.hip.h): values are canonical blst_fr images (x 2^256, below r); u_i, gamma^i and the powers of r carry 2^270
// (prepared by the host, canonical), so a product of a value and a multiplier is a value.
#include <hip/hip_runtime.h>

#include "combine_lanes.hip.h"
#include "engine.h"
#include "fr30.hip.h"

namespace kzg {

namespace {

struct MlLimbs {
    uint32_t l[8];
};

// multiplier i of the kernel's argument, held in vector registers: nine digits per level in scalar registers, with every level's
// loads hoisted to the kernel's start, made the compiler spill scalar registers in k_ml_fold
__device__ __forceinline__ Fr30 ml_mult(const MlMultipliers& t, uint32_t i) {
    Fr30 v;
#pragma unroll
    for (int k = 0; k < kR9; k++) {
        v.d[k] = t.m[i][k];
        asm volatile("" : "+v"(v.d[k]));
    }
    return v;
}
__device__ __forceinline__ MlLimbs ml_load(const uint32_t* __restrict__ src, uint64_t idx, uint64_t len) {
    MlLimbs v;
    if (idx < len) {
        const uint4* p = reinterpret_cast<const uint4*>(src) + 2 * idx;
        const uint4 a = p[0], b = p[1];
        v.l[0] = a.x; v.l[1] = a.y; v.l[2] = a.z; v.l[3] = a.w;
        v.l[4] = b.x; v.l[5] = b.y; v.l[6] = b.z; v.l[7] = b.w;
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++) v.l[k] = 0u;
    }
    return v;
}
__device__ __forceinline__ void ml_store(uint32_t* dst, uint64_t idx, const MlLimbs& v) {
    uint4* q = reinterpret_cast<uint4*>(dst) + 2 * idx;
    q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}
// One fold, canonical in and canonical out: a + u (b - a).
// Bound.  a, b are canonical (0 <= a, b < r), carry-normalised on load (fr30_from_limbs: digits within [-2^29 - 4, 2^29 + 4]).
// d = b - a is a raw difference of two such values: digits within 2^30 + 8, the operand fr30_mul takes as "a raw sum of two",
// |d| < r.  u is canonical and carry-normalised, so p = u d / 2^270 has digits 0..7 in [-2^29, 2^29) and
// |p| <= 0.5001 r + r r / 2^270 < 0.5002 r.  a + p (raw: digits within 2^30 + 4, the sequential carry of fr30_to_limbs takes
// any int32 digits of that size) lies in (-0.5002 r, 1.5002 r), inside the (-r, 2r) that fr30_to_limbs canonicalises with one
// conditional + r and one conditional - r.  So a value never grows along a chain of folds: it is REDUCED TO CANONICAL FORM AFTER
// EVERY FOLD (a carry pass and two conditional additions, a fraction of a product), the same limbs are stored to the pyramid
// and fed to the next level, and the k-th fold of a chain meets exactly the magnitudes of the first.  Every u_i < r gives the
// exact residue, 0, 1, r - 1 and (r + 1) / 2 included: nothing above depends on the value of u.
__device__ __forceinline__ MlLimbs ml_fold1(const MlLimbs& a, const MlLimbs& b, const Fr30& u) {
    const Fr30 fa = fr30_from_limbs(a.l), fb = fr30_from_limbs(b.l);
    Fr30 d;
#pragma unroll
    for (int k = 0; k < kR9; k++) d.d[k] = fb.d[k] - fa.d[k];
    const Fr30 s = fr30_add_raw(fa, fr30_mul(u, d));
    MlLimbs o;
    fr30_to_limbs(s, o.l);
    return o;
}
__device__ __forceinline__ MlLimbs ml_shfl_down(const MlLimbs& v, int delta) {
    MlLimbs o;
#pragma unroll
    for (int k = 0; k < 8; k++) o.l[k] = (uint32_t)__shfl_down((int)v.l[k], delta, 64);
    return o;
}

// src: `len` canonical values (a power of two), level `first` of the call; this launch writes the levels first + 1 ..
// first + nlev (nlev = min(11, log2 len) >= 1) into the pyramid of n values' polynomial.  Tile b covers the source indices
// [2048 b, 2048 b + 2048); an index past len reads as zero and no value past a level's length is stored.
__global__ void __launch_bounds__(kMlThreads) k_ml_fold(const uint32_t* __restrict__ src, uint32_t len, uint32_t first, uint32_t nlev,
                                                        uint32_t n, const MlMultipliers us, uint32_t* __restrict__ pyr) {
    __shared__ uint32_t lds[4][8];
    const uint32_t t = threadIdx.x, tile = blockIdx.x;
    const uint64_t base = (uint64_t)tile * kMlTile + 8u * t;
    // where level first + j of this tile begins in the pyramid, and how many values the level has
    auto level_at = [&](uint32_t j) { return (uint64_t)n - (uint64_t)(n >> (first + j - 1)) + (uint64_t)tile * (kMlTile >> j); };
    MlLimbs v[8];
#pragma unroll
    for (int m = 0; m < 8; m++) v[m] = ml_load(src, base + m, len);
    // three levels in the lane
    {
        const Fr30 u = ml_mult(us, first);
#pragma unroll
        for (int m = 0; m < 4; m++) {
            v[m] = ml_fold1(v[2 * m], v[2 * m + 1], u);
            const uint64_t q = 4u * t + m;
            if ((uint64_t)tile * (kMlTile >> 1) + q < (len >> 1)) ml_store(pyr, level_at(1) + q, v[m]);
        }
    }
    if (nlev >= 2) {
        const Fr30 u = ml_mult(us, first + 1);
#pragma unroll
        for (int m = 0; m < 2; m++) {
            v[m] = ml_fold1(v[2 * m], v[2 * m + 1], u);
            const uint64_t q = 2u * t + m;
            if ((uint64_t)tile * (kMlTile >> 2) + q < (len >> 2)) ml_store(pyr, level_at(2) + q, v[m]);
        }
    }
    if (nlev >= 3) {
        const Fr30 u = ml_mult(us, first + 2);
        v[0] = ml_fold1(v[0], v[1], u);
        if ((uint64_t)tile * (kMlTile >> 3) + t < (len >> 3)) ml_store(pyr, level_at(3) + t, v[0]);
    }
    // six levels across the wave: at step s the lanes whose low s + 1 bits are zero fold their value with the one 2^s lanes up
    // (the other lanes compute a value nobody reads: the branch is uniform, the shuffle sees every lane)
    MlLimbs w = v[0];
#pragma unroll 1
    for (uint32_t s = 0; s < 6; s++) {
        const uint32_t j = 4 + s;  // the level this step writes, counted from `first`
        if (j > nlev) break;
        const MlLimbs o = ml_shfl_down(w, 1 << s);
        w = ml_fold1(w, o, ml_mult(us, first + j - 1));
        const uint32_t q = t >> (s + 1);
        if ((t & ((2u << s) - 1u)) == 0 && (uint64_t)tile * (kMlTile >> j) + q < (len >> j)) ml_store(pyr, level_at(j) + q, w);
    }
    // two levels across the four waves
    if (nlev >= 10) {  // (uniform)
        if ((t & 63u) == 0) {
#pragma unroll
            for (int k = 0; k < 8; k++) lds[t >> 6][k] = w.l[k];
        }
        __syncthreads();
        if (t == 0) {
            MlLimbs a[4];
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int k = 0; k < 8; k++) a[i].l[k] = lds[i][k];
            const Fr30 u9 = ml_mult(us, first + 9);
            a[0] = ml_fold1(a[0], a[1], u9);
            a[1] = ml_fold1(a[2], a[3], u9);
            if ((uint64_t)tile * 2 < (len >> 10)) ml_store(pyr, level_at(10), a[0]);
            if ((uint64_t)tile * 2 + 1 < (len >> 10)) ml_store(pyr, level_at(10) + 1, a[1]);
            if (nlev >= 11) {
                a[0] = ml_fold1(a[0], a[1], ml_mult(us, first + 10));
                if ((uint64_t)tile < (len >> 11)) ml_store(pyr, level_at(11), a[0]);
            }
        }
    }
}
static_assert(kMlTile == 2048 && kMlThreads == 256, "k_ml_fold: eight values per lane, 3 + 6 + 2 levels");

__device__ __forceinline__ void ml_store_record(uint32_t* p, const Fr30& e) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4((uint32_t)e.d[0], (uint32_t)e.d[1], (uint32_t)e.d[2], (uint32_t)e.d[3]);
    q[1] = make_uint4((uint32_t)e.d[4], (uint32_t)e.d[5], (uint32_t)e.d[6], (uint32_t)e.d[7]);
    q[2] = make_uint4((uint32_t)e.d[8], 0u, 0u, 0u);
}

// The walk over a lane's eight indices from the top, unrolled by recursion over the index (a rolled loop would index lo / hi in
// scratch): both Horner chains take the coefficient, h in r^256 and g in (r^2)^256; an index past len counts as zero
template <int M>
__device__ __forceinline__ void ml_eval_steps(Fr30& h, Fr30& g, const uint4 (&lo)[8], const uint4 (&hi)[8], const Fr30& z256,
                                              const Fr30& s256, uint64_t base, uint32_t len) {
    Fr30 c = fr30_from_u4(lo[M], hi[M]);
    if (base + (uint64_t)M * kCombineThreads >= len) c = fr30_zero();
    h = fr30_add_raw(fr30_mul(h, z256), c);
    g = fr30_add_raw(fr30_mul(g, s256), c);
    if constexpr (M > 0) ml_eval_steps<M - 1>(h, g, lo, hi, z256, s256, base, len);
}

// blockIdx.y = level i (f_0 at evals, f_i at its place in the pyramid, n >> i values), blockIdx.x = tile of 2048 indices; tab:
// the 66 powers of r (k_combine_eval's layout), then the 66 powers of r^2.  Record (i, p, tile) at 12 ((3 i + p) tiles0 + tile)
// words, tiles0 = gridDim.x.
// Bound.  Horner: h = h z^256 + c with c canonical and carry-normalised: the raw sum of a product (|.| <= 0.5001 r + small,
// digits 0..7 in [-2^29, 2^29)) and c is an operand fr30_mul takes as it is (k_combine_eval's chain, unchanged).  The lane's
// share h z^t is a product again, and so is its negation (the digit ranges are symmetric up to one unit, inside the
// carry-normalised range cmb_workgroup_sum asks for): each record is a carry-normalised sum of 256 values of magnitude
// <= 0.5001 r + r / 2^14, below 128.1 r, its top digit below kR9SumTopBound = 2^22 -- what cmb_tiles_sum takes.
__global__ void __launch_bounds__(kCombineThreads) k_ml_eval(const uint32_t* __restrict__ evals, const uint32_t* __restrict__ pyr,
                                                             uint32_t n, const Fr30* __restrict__ tab,
                                                             uint32_t* __restrict__ partial) {
    __shared__ int32_t lds[kR9][4];
    const uint32_t t = threadIdx.x, tile = blockIdx.x, tiles0 = gridDim.x, i = blockIdx.y;
    const uint32_t len = n >> i;
    if ((uint64_t)tile * kCombineTile >= len) return;  // (the whole workgroup)
    const uint4* src = reinterpret_cast<const uint4*>(i == 0 ? evals : pyr + 8 * ((uint64_t)n - (uint64_t)(n >> (i - 1))));
    const uint64_t base = (uint64_t)tile * kCombineTile + t;
    uint4 lo[8], hi[8];
#pragma unroll
    for (int m = 0; m < 8; m++) {
        const uint64_t idx = base + (uint64_t)m * kCombineThreads;
        const uint4* p = src + 2 * (idx < len ? idx : 0);  // (len >= 1; counted as zero below)
        lo[m] = p[0];
        hi[m] = p[1];
    }
    const Fr30* tab2 = tab + kCombineTabGamma;
    const Fr30 z256 = fr30_table(tab, kCombineTabZ256), s256 = fr30_table(tab2, kCombineTabZ256);
    Fr30 h = fr30_zero(), g = fr30_zero();
    ml_eval_steps<7>(h, g, lo, hi, z256, s256, base, len);
    const Fr30 zt = fr30_mul(fr30_table(tab, kCombineTabPa + (t >> 4)), fr30_table(tab, kCombineTabPb + (t & 15)));
    const Fr30 st = fr30_mul(fr30_table(tab2, kCombineTabPa + (t >> 4)), fr30_table(tab2, kCombineTabPb + (t & 15)));
    const Fr30 a = fr30_mul(h, zt);
    Fr30 b;
#pragma unroll
    for (int k = 0; k < kR9; k++) b.d[k] = (t & 1u) ? -a.d[k] : a.d[k];
    const Fr30 e0 = cmb_workgroup_sum(a, lds);
    const Fr30 e1 = cmb_workgroup_sum(b, lds);
    const Fr30 e2 = cmb_workgroup_sum(fr30_mul(g, st), lds);
    if (t == 0) {
        ml_store_record(partial + ((size_t)(3 * i + 0) * tiles0 + tile) * kCombinePartialWords, e0);
        ml_store_record(partial + ((size_t)(3 * i + 1) * tiles0 + tile) * kCombinePartialWords, e1);
        ml_store_record(partial + ((size_t)(3 * i + 2) * tiles0 + tile) * kCombinePartialWords, e2);
    }
}

// workgroup 3 i + p: out[3 i + p] = sum_tile record(i, p, tile) W^tile, W = r^2048 for p < 2 (2048 is even: the same step serves
// -r), (r^2)^2048 for p = 2.  The bound is k_combine_eval_finish's.
__global__ void __launch_bounds__(kCombineThreads) k_ml_eval_finish(const uint32_t* __restrict__ partial, uint32_t n, uint32_t tiles0,
                                                                    const Fr30* __restrict__ tab, uint32_t* __restrict__ out) {
    __shared__ int32_t lds[kR9][4];
    const uint32_t b = blockIdx.x, i = b / 3, p = b % 3;
    const uint32_t tiles = ((n >> i) + kCombineTile - 1) / kCombineTile;
    const Fr30 y = cmb_tiles_sum(partial + (size_t)b * tiles0 * kCombinePartialWords, tiles, p == 2 ? tab + kCombineTabGamma : tab, lds);
    if (threadIdx.x == 0) fr30_store(out + 8 * (size_t)b, fr30_sum_reduce(y));
}

// F[j] = f_0[j] + sum_{1 <= i < l, j < n >> i} gamma^i f_i[j], one index per lane.
// Bound (fr30.hip.h, fr30_mac): the accumulator starts as the canonical f_0[j] and takes at most l - 1 <= 21 products of a canonical
// value and a canonical multiplier, carry-normalised after every one: well inside the 256 products of fr30_mac's contract (the
// sum stays below 11.6 r, its top digit below 2^19 < kR9SumTopBound); fr30_sum_reduce brings it under 0.51 r for fr30_to_limbs.
__global__ void __launch_bounds__(kMlThreads) k_ml_combine(const uint32_t* __restrict__ evals, const uint32_t* __restrict__ pyr,
                                                           uint32_t n, uint32_t ell, const MlMultipliers gam, uint32_t* __restrict__ f) {
    const uint64_t j = (uint64_t)blockIdx.x * kMlThreads + threadIdx.x;
    if (j >= n) return;
    const MlLimbs c0 = ml_load(evals, j, n);
    Fr30 acc = fr30_from_limbs(c0.l);
#pragma unroll 1
    for (uint32_t i = 1; i < ell && j < (n >> i); i++) {
        const MlLimbs c = ml_load(pyr, (uint64_t)n - (uint64_t)(n >> (i - 1)) + j, (uint64_t)n);
        acc = fr30_mac(acc, fr30_from_limbs(c.l), ml_mult(gam, i));
    }
    fr30_store(f + 8 * j, fr30_sum_reduce(acc));
}

}  // namespace

void launch_ml_fold(hipStream_t s, const uint32_t* d_evals, uint32_t ell, const MlMultipliers& us, uint32_t* d_pyr) {
    const uint32_t n = 1u << ell;
    const uint32_t nlev1 = ell < kMlLevels ? ell : kMlLevels;
    hipLaunchKernelGGL(k_ml_fold, dim3((n + kMlTile - 1) / kMlTile), dim3(kMlThreads), 0, s, d_evals, n, 0u, nlev1, n, us, d_pyr);
    if (ell > kMlLevels) {  // level 11: n >> 11 <= 2048 values, one workgroup takes them down to f_l
        const uint32_t* lvl = d_pyr + 8 * ((size_t)n - (n >> (kMlLevels - 1)));
        hipLaunchKernelGGL(k_ml_fold, dim3(1), dim3(kMlThreads), 0, s, lvl, n >> kMlLevels, kMlLevels, ell - kMlLevels, n, us, d_pyr);
    }
}

void launch_ml_eval(hipStream_t s, const uint32_t* d_evals, const uint32_t* d_pyr, uint32_t ell, const Fr30* d_tab,
                    uint32_t* d_partial, uint32_t* d_ys) {
    const uint32_t n = 1u << ell, tiles0 = combine_tiles(n);
    hipLaunchKernelGGL(k_ml_eval, dim3(tiles0, ell), dim3(kCombineThreads), 0, s, d_evals, d_pyr, n, d_tab, d_partial);
    hipLaunchKernelGGL(k_ml_eval_finish, dim3(3 * ell), dim3(kCombineThreads), 0, s, (const uint32_t*)d_partial, n, tiles0, d_tab, d_ys);
}

void launch_ml_combine(hipStream_t s, const uint32_t* d_evals, const uint32_t* d_pyr, uint32_t ell, const MlMultipliers& gam,
                       uint32_t* d_f) {
    const uint32_t n = 1u << ell;
    hipLaunchKernelGGL(k_ml_combine, dim3((n + kMlThreads - 1) / kMlThreads), dim3(kMlThreads), 0, s, d_evals, d_pyr, n, ell, gam, d_f);
}

}  // namespace kzg
