// recover_kernels.hip -- every coefficient of a batch of polynomials from part of their cells (kzg_recover_cells_and_proofs;
// DESIGN.md section 4.9).
//
// Domain of N = 2^K points, cells of l = 2^t, M = N / l cells; cell j is {w_N^(j + M i) : i < l} and X^l = a_j = w_M^j on
// it.  S = the missing cells, Z'(Y) = prod_{j in S} (Y - w_M^j), Z(X) = Z'(X^l) vanishes on exactly the missing points.
// With g = 7 (neither g w_N^e nor g^l w_M^e is a root of Z or Z'), per polynomial:
//     D[j + M i] = E_j[i] Z'(w_M^j) (received j), 0 (missing j)          k_rec_scatter
//     PZ = INTT_N(D)                                                     k_fr_stage (fk20_kernels.hip), inverse tables
//     PZ_i g^i / N,  NTT_N,  x 1/Z'(g^l w_M^(e mod M)),  INTT_N             k_rec_twist, k_fr_stage, k_rec_divide, k_fr_stage
//     P_i = v_i g^-i / N: i < n written out, any non-zero i >= n flags the polynomial     k_rec_untwist
// and, for the cells, NTT_N of P padded to N gathered cell-major (k_rec_gather).  Z'(w_M^i) and 1/Z'(g^l w_M^i) are shared by
// the batch: k_rec_vanish forms products over chunks of the missing list (2M points x parts lanes), k_rec_vanish_fold
// multiplies the parts of each point and inverts the coset half by Fermat (a^(r-2), one lane per value).
//
// Forms (fr30.hip.h).  Data values are blst_fr images (x 2^256), stored canonical.  Everything the host or the vanishing
// kernels prepare as a multiplier is "x 2^270" (fr30_arg_from_mont256): the twiddles (w_N^e = hi[e' >> 11] lo[e' & 2047],
// e' = e 2^(22 - K), as cell_kernels.hip), the g-power tables of the same shape (g^i, g^-i, i < 2^22), g^l, 1/N.  fr30_mul of
// two multipliers is a multiplier, so Z' and its inverse are formed in that form and stored canonical, and fr30_mul(value,
// multiplier) is a value.
//
// Bounds.  A loaded canonical value, table entry or stored multiplier is below 2^256 with carry-normalised digits: a valid
// fr30_mul operand.  Every fr30_mul result here has |v| <= 0.5001 r + |a b| / 2^270 < 0.5002 r (|a|, |b| < 2^256 or products
// themselves), inside (-r, 2r), which fr30_to_limbs reduces to the canonical residue.  A factor y - w_M^j is the carry-
// normalised difference of two products, |y - w| < 1.0004 r < 2^256.  The transform stages are k_fr_stage's (canonical in
// and out, one product each).
#include <hip/hip_runtime.h>

#include "engine.h"
#include "fr30.hip.h"
#include "fr30_lanes.hip.h"

namespace kzg {

namespace {

constexpr uint32_t kRecThreads = 256;

// canonical 8 x u32; returns whether the residue is non-zero
__device__ __forceinline__ bool rec_store(uint32_t* __restrict__ p, const Fr30& v) {
    uint32_t l[8];
    fr30_to_limbs(v, l);
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(l[0], l[1], l[2], l[3]);
    q[1] = make_uint4(l[4], l[5], l[6], l[7]);
    return (l[0] | l[1] | l[2] | l[3] | l[4] | l[5] | l[6] | l[7]) != 0;
}
// w_M^i = w_N^(i l) from the forward NTT twiddles
__device__ __forceinline__ Fr30 rec_root_m(const Fr30* __restrict__ tw, uint32_t log_n, uint32_t log_l, uint32_t i) {
    return fr30_pow22(tw, (i << log_l) << (kNttMaxLog - log_n));
}

// lane (part q, point p): out[q 2M + p] = prod_{s in part q} (y_p - w_M^missing[s]); y_p = w_M^p (p < M), g^l w_M^(p - M)
__global__ void __launch_bounds__(kRecThreads) k_rec_vanish(const uint32_t* __restrict__ missing, uint32_t n_missing,
                                                            uint32_t per_part, uint32_t parts, const Fr30* __restrict__ tw,
                                                            uint32_t log_n, uint32_t log_l, Fr30 gl, uint32_t* __restrict__ out) {
    const uint32_t log_m = log_n - log_l;
    const uint32_t points = 2u << log_m;
    const uint32_t t = blockIdx.x * kRecThreads + threadIdx.x;
    if (t >= points * parts) return;
    const uint32_t p = t & (points - 1), q = t >> (log_m + 1);
    Fr30 y = rec_root_m(tw, log_n, log_l, p & ((1u << log_m) - 1));
    if (p >> log_m) y = fr30_mul(y, gl);
    Fr30 acc = fr30_const_one270();
    const uint32_t s1 = (q + 1) * per_part < n_missing ? (q + 1) * per_part : n_missing;
#pragma unroll 1
    for (uint32_t s = q * per_part; s < s1; s++) {
        const Fr30 w = rec_root_m(tw, log_n, log_l, missing[s]);
        Fr30 d;
#pragma unroll
        for (int i = 0; i < kR9; i++) d.d[i] = y.d[i] - w.d[i];
        acc = fr30_mul(acc, fr30_norm(d));
    }
    rec_store(out + 8 * (size_t)t, acc);
}

// point p: the product of its parts; the coset half (p >= M) inverted, a^(r - 2) by square and multiply -> z[8 p]
__global__ void __launch_bounds__(kRecThreads) k_rec_vanish_fold(const uint32_t* __restrict__ part, uint32_t parts, uint32_t log_m,
                                                                 uint32_t* __restrict__ z) {
    const uint32_t points = 2u << log_m;
    const uint32_t p = blockIdx.x * kRecThreads + threadIdx.x;
    if (p >= points) return;
    Fr30 a = fr30_load(part + 8 * (size_t)p);
#pragma unroll 1
    for (uint32_t q = 1; q < parts; q++) a = fr30_mul(a, fr30_load(part + 8 * ((size_t)q * points + p)));
    if (p >> log_m) {
        // r - 2, little-endian u32
        constexpr uint32_t E[8] = {0xffffffffu, 0xfffffffeu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
        Fr30 acc = fr30_const_one270();
#pragma unroll 1
        for (int bit = 254; bit >= 0; bit--) {
            acc = fr30_mul(acc, acc);
            if ((E[bit >> 5] >> (bit & 31)) & 1) acc = fr30_mul(acc, a);
        }
        a = acc;
    }
    rec_store(z + 8 * (size_t)p, a);
}

// lane (b, e), e = j + M i: D[b N + e] = E_(b, pos[j])[i] Z'(w_M^j), or 0 where pos[j] < 0 (a missing cell)
__global__ void __launch_bounds__(kRecThreads) k_rec_scatter(const uint32_t* __restrict__ cells, const int32_t* __restrict__ pos,
                                                             const uint32_t* __restrict__ zrecv, uint32_t k, uint32_t log_n,
                                                             uint32_t log_l, uint64_t lanes, uint32_t* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * kRecThreads + threadIdx.x;
    if (t >= lanes) return;
    const uint32_t log_m = log_n - log_l;
    const uint32_t e = (uint32_t)t & ((1u << log_n) - 1);
    const uint64_t b = t >> log_n;
    const uint32_t j = e & ((1u << log_m) - 1), i = e >> log_m;
    const int32_t at = pos[j];
    if (at < 0) {
        uint4* q = reinterpret_cast<uint4*>(out + 8 * t);
        q[0] = q[1] = make_uint4(0, 0, 0, 0);
        return;
    }
    const Fr30 v = fr30_load(cells + 8 * (((b * k + (uint32_t)at) << log_l) + i));
    rec_store(out + 8 * t, fr30_mul(v, fr30_load(zrecv + 8 * (size_t)j)));
}

// in place: v[b N + i] *= g^i c (c = 1/N, multiplier form)
__global__ void __launch_bounds__(kRecThreads) k_rec_twist(uint32_t* __restrict__ io, uint32_t log_n, uint64_t lanes,
                                                           const Fr30* __restrict__ gtab, Fr30 c) {
    const uint64_t t = (uint64_t)blockIdx.x * kRecThreads + threadIdx.x;
    if (t >= lanes) return;
    const uint32_t i = (uint32_t)t & ((1u << log_n) - 1);
    const Fr30 m = fr30_mul(fr30_pow22(gtab, i), c);
    rec_store(io + 8 * t, fr30_mul(fr30_load(io + 8 * t), m));
}

// in place: v[b N + e] *= 1/Z'(g^l w_M^(e mod M)) (zinv: M stored multipliers)
__global__ void __launch_bounds__(kRecThreads) k_rec_divide(uint32_t* __restrict__ io, uint32_t log_m, uint64_t lanes,
                                                            const uint32_t* __restrict__ zinv) {
    const uint64_t t = (uint64_t)blockIdx.x * kRecThreads + threadIdx.x;
    if (t >= lanes) return;
    const uint32_t e = (uint32_t)t & ((1u << log_m) - 1);
    rec_store(io + 8 * t, fr30_mul(fr30_load(io + 8 * t), fr30_load(zinv + 8 * (size_t)e)));
}

// lane (b, i): P_i = v[b N + i] g^-i c.  i < n: to coef[b n + i]; pad (may be null): P padded to N in place of v;
// a non-zero P_i with i >= n sets flags[b]
__global__ void __launch_bounds__(kRecThreads) k_rec_untwist(uint32_t* __restrict__ io, uint32_t log_n, uint32_t n, uint64_t lanes,
                                                             const Fr30* __restrict__ ginv, Fr30 c, uint32_t* __restrict__ coef,
                                                             int pad, uint32_t* __restrict__ flags) {
    const uint64_t t = (uint64_t)blockIdx.x * kRecThreads + threadIdx.x;
    if (t >= lanes) return;
    const uint32_t i = (uint32_t)t & ((1u << log_n) - 1);
    const uint64_t b = t >> log_n;
    const Fr30 v = fr30_mul(fr30_mul(fr30_load(io + 8 * t), fr30_pow22(ginv, i)), c);
    if (i < n) {
        rec_store(coef + 8 * (b * n + i), v);
        if (pad) rec_store(io + 8 * t, v);
        return;
    }
    if (!fr30_is_zero(v)) flags[b] = 1u;  // plain store: every writer stores 1
    if (pad) {
        uint4* q = reinterpret_cast<uint4*>(io + 8 * t);
        q[0] = q[1] = make_uint4(0, 0, 0, 0);
    }
}

// out[b N + j l + i] = in[b N + j + M i]: natural order into cells (k_cells_gather for a batch)
__global__ void __launch_bounds__(kRecThreads) k_rec_gather(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                            uint32_t log_n, uint32_t log_l, uint64_t lanes) {
    const uint64_t t = (uint64_t)blockIdx.x * kRecThreads + threadIdx.x;
    if (t >= lanes) return;
    const uint32_t o = (uint32_t)t & ((1u << log_n) - 1);
    const uint64_t base = t - o;
    const uint32_t j = o >> log_l, i = o & ((1u << log_l) - 1u);
    const uint4* src = reinterpret_cast<const uint4*>(in) + 2 * (base + j + ((uint64_t)i << (log_n - log_l)));
    uint4* dst = reinterpret_cast<uint4*>(out) + 2 * t;
    dst[0] = src[0];
    dst[1] = src[1];
}

dim3 rec_grid(uint64_t lanes) { return dim3((unsigned)((lanes + kRecThreads - 1) / kRecThreads)); }

}  // namespace

uint32_t recover_vanish_parts(uint32_t n_missing) {
    // about 256 factors per lane, at most 16 parts (16 x 2M lanes); at least one part even when nothing is missing
    uint32_t parts = (n_missing + 255) / 256;
    return parts < 1 ? 1 : (parts > 16 ? 16 : parts);
}

void launch_recover_vanishing(hipStream_t s, const uint32_t* d_missing, uint32_t n_missing, const void* d_tw, uint32_t log_n,
                              uint32_t log_l, const Fr30& gl, uint32_t* d_part, uint32_t* d_z) {
    const uint32_t log_m = log_n - log_l;
    const uint32_t parts = recover_vanish_parts(n_missing);
    const uint32_t per = (n_missing + parts - 1) / parts;
    const uint64_t lanes = (uint64_t)parts << (log_m + 1);
    hipLaunchKernelGGL(k_rec_vanish, rec_grid(lanes), dim3(kRecThreads), 0, s, d_missing, n_missing, per, parts, (const Fr30*)d_tw,
                       log_n, log_l, gl, d_part);
    hipLaunchKernelGGL(k_rec_vanish_fold, rec_grid(2u << log_m), dim3(kRecThreads), 0, s, (const uint32_t*)d_part, parts, log_m, d_z);
}

void launch_recover_scatter(hipStream_t s, const uint32_t* d_cells, const int32_t* d_pos, const uint32_t* d_zrecv, uint32_t k,
                            uint32_t log_n, uint32_t log_l, uint64_t batch, uint32_t* d_out) {
    const uint64_t lanes = batch << log_n;
    hipLaunchKernelGGL(k_rec_scatter, rec_grid(lanes), dim3(kRecThreads), 0, s, d_cells, d_pos, d_zrecv, k, log_n, log_l, lanes, d_out);
}

void launch_recover_twist(hipStream_t s, uint32_t* d_io, uint32_t log_n, uint64_t batch, const void* d_gtab, const Fr30& c) {
    const uint64_t lanes = batch << log_n;
    hipLaunchKernelGGL(k_rec_twist, rec_grid(lanes), dim3(kRecThreads), 0, s, d_io, log_n, lanes, (const Fr30*)d_gtab, c);
}

void launch_recover_divide(hipStream_t s, uint32_t* d_io, uint32_t log_n, uint32_t log_l, uint64_t batch, const uint32_t* d_zinv) {
    const uint64_t lanes = batch << log_n;
    hipLaunchKernelGGL(k_rec_divide, rec_grid(lanes), dim3(kRecThreads), 0, s, d_io, log_n - log_l, lanes, d_zinv);
}

void launch_recover_untwist(hipStream_t s, uint32_t* d_io, uint32_t log_n, uint32_t n, uint64_t batch, const void* d_ginv,
                            const Fr30& c, uint32_t* d_coef, bool pad, uint32_t* d_flags) {
    const uint64_t lanes = batch << log_n;
    hipLaunchKernelGGL(k_rec_untwist, rec_grid(lanes), dim3(kRecThreads), 0, s, d_io, log_n, n, lanes, (const Fr30*)d_ginv, c,
                       d_coef, pad ? 1 : 0, d_flags);
}

void launch_recover_gather(hipStream_t s, const uint32_t* d_in, uint32_t* d_out, uint32_t log_n, uint32_t log_l, uint64_t batch) {
    const uint64_t lanes = batch << log_n;
    hipLaunchKernelGGL(k_rec_gather, rec_grid(lanes), dim3(kRecThreads), 0, s, d_in, d_out, log_n, log_l, lanes);
}

}  // namespace kzg
