// ntt_kernels.hip -- number-theoretic transform over the power-of-two subgroups of Fr (kzg_ntt, kzg_commit_evaluations,
// kzg_open_evaluations): evals[i] = sum_j c[j] w^(i j), natural order on both sides, data in the ABI's "x 2^256" form.
//
// Layout (Stockham autosort, radix 2^m per pass).  Pass p with Ns = product of the earlier radices
// and R = 2^m reads v_r = in[j + r N/R] (r < R) for each j < N/R, computes the R-point DFT of (v_r w_{Ns R}^((j mod Ns) r)),
// and writes its output r to out[(j / Ns) Ns R + (j mod Ns) + r Ns].  The input twiddle of pass p + 1 depends only on
// the index o that pass p writes, so pass p multiplies by it before the store: every value that reaches memory is a
// product.  The last pass multiplies by a constant instead (1, or 1/n for the inverse).  No separate reordering step:
// the R-point DFT runs in LDS as in-place radix-2 DIT stages over a tile loaded in bit-reversed LDS order.
//
// Bounds (fr30.hip.h's conventions).  A loaded value is an integer below 2^256 < 2.3 r (canonical for every pass but the
// first, and for the first whenever the caller respects the ABI).  The first stage of a tile has twiddle 1: |v| < 4.6 r.
// Every later stage adds a product (|w b| <= 0.5001 r + |w b| / 2^270 < 0.5002 r for |b| < 2^259) to one half and
// subtracts it from the other: after m <= 11 stages |v| < 4.6 r + 10 * 0.5002 r < 10 r < 2^259.  Every add / sub is
// carry-normalised (fr30_norm: digits of two normalised operands sum to < 2^30 + 8 < 2^31 - 2^29), so digits 0..7 stay in
// [-2^29 - 4, 2^29 + 4] and the top digit below 2^20: inside fr30_mul's operand bound.  The closing product brings every
// value back to |v| <= 0.5002 r, inside (-r, 2r), which fr30_to_limbs reduces to the canonical residue.
//
// Twiddles: two tables of 2048 entries per direction, lo[i] = w^i and hi[i] = w^(2048 i) for w = w_(2^22), in
// fr30_mul's multiplier form (x 2^270, fr30_arg_from_mont256).  w_N^e = w_(2^22)^(e 2^22 / N) = hi[e >> 11] * lo[e & 2047]:
// one extra product per stored value.  The stage twiddles w_(2h)^k (2h <= 2048) are hi[k 2048 / 2h] directly.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "fr30.hip.h"
#include "fr30_lanes.hip.h"

namespace kzg {

namespace {

constexpr uint32_t kNttThreads = 256;

__device__ __forceinline__ Fr30 lds_get(const int32_t* lds, uint32_t T, uint32_t pos) {
    Fr30 v;
#pragma unroll
    for (int i = 0; i < kR9; i++) v.d[i] = lds[i * T + pos];
    return v;
}
__device__ __forceinline__ void lds_put(int32_t* lds, uint32_t T, uint32_t pos, const Fr30& v) {
#pragma unroll
    for (int i = 0; i < kR9; i++) lds[i * T + pos] = v.d[i];
}

// One Stockham pass over a tile of J = 2^log_j consecutive j and R = 2^m values each (T = J R <= kNttTile), LDS as nine
// digit planes of T words.  tw: lo[2048] then hi[2048] of the direction.  next_m: the radix of the next pass (0: last
// pass, every output is multiplied by last_c instead).  in and out may be the same buffer when the whole transform is
// this one workgroup (a single pass: kzg_ntt's staging buffer, kzg_ntt_device with d_in == d_out), so neither is
// __restrict__: every load of the tile comes before the first __syncthreads and every store after the last.
__global__ void __launch_bounds__(kNttThreads) k_ntt_pass(const uint32_t* in, uint32_t* out,
                                                          const Fr30* __restrict__ tw, uint32_t log_n, uint32_t m,
                                                          uint32_t log_ns, uint32_t log_j, uint32_t next_m, Fr30 last_c) {
    extern __shared__ int32_t lds[];
    const uint32_t T = 1u << (m + log_j);
    const uint32_t R = 1u << m;
    const uint32_t J = 1u << log_j;
    const uint32_t j0 = blockIdx.x << log_j;
    const Fr30* __restrict__ lo = tw;
    const Fr30* __restrict__ hi = tw + kNttTableLen;

    // load: runs of J consecutive j per r (coalesced), stored at the bit-reversed position of r
    for (uint32_t t = threadIdx.x; t < T; t += kNttThreads) {
        const uint32_t jj = t & (J - 1), rr = t >> log_j;
        const uint64_t idx = (uint64_t)(j0 + jj) + ((uint64_t)rr << (log_n - m));
        const uint4* p = reinterpret_cast<const uint4*>(in) + 2 * idx;
        const uint4 a = p[0], b = p[1];
        const uint32_t l[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        const uint32_t pos = (jj << m) + (m ? (__brev(rr) >> (32 - m)) : 0u);
        lds_put(lds, T, pos, fr30_from_limbs(l));
    }
    // radix-2 DIT stages in place; stage s pairs positions p0 and p0 + h (h = 2^s) with twiddle w_(2h)^k
    for (uint32_t s = 0; s < m; s++) {
        __syncthreads();
        const uint32_t h = 1u << s;
        for (uint32_t b = threadIdx.x; b < T / 2; b += kNttThreads) {
            const uint32_t jj = b >> (m - 1), q = b & (R / 2 - 1);
            const uint32_t k = q & (h - 1);
            const uint32_t p0 = (jj << m) + ((q >> s) << (s + 1)) + k, p1 = p0 + h;
            const Fr30 x = lds_get(lds, T, p0);
            Fr30 y = lds_get(lds, T, p1);
            if (s) y = fr30_mul(y, fr30_table(hi, k << (10 - s)));
            lds_put(lds, T, p0, fr30_add(x, y));
            lds_put(lds, T, p1, fr30_sub(x, y));
        }
    }
    __syncthreads();
    // store: output r of DFT j goes to o = (j / Ns) Ns R + (j mod Ns) + r Ns.  The first pass (Ns = 1) writes the tile as
    // one contiguous run (o = j R + r): r is the fast index there; later passes have Ns >= J and j is the fast index.
    const uint32_t Ns = 1u << log_ns;
    for (uint32_t t = threadIdx.x; t < T; t += kNttThreads) {
        const uint32_t jj = log_ns == 0 ? (t >> m) : (t & (J - 1));
        const uint32_t rr = log_ns == 0 ? (t & (R - 1)) : (t >> log_j);
        const uint32_t j = j0 + jj;
        const uint32_t o = ((j >> log_ns) << (log_ns + m)) + (j & (Ns - 1)) + (rr << log_ns);
        Fr30 v = lds_get(lds, T, (jj << m) + rr);
        if (next_m) {
            // the next pass reads o as j' = o mod (N / R'), r' = o / (N / R') with Ns' = Ns R: twiddle w_(Ns' R')^((j' mod Ns') r'),
            // i.e. w_(2^22)^e with e = ((j' mod Ns') r') 2^(22 - log Ns' - m') < 2^22
            const uint32_t log_ns2 = log_ns + m;
            const uint32_t r2 = o >> (log_n - next_m);
            const uint32_t j2 = o & ((1u << log_ns2) - 1);  // (o mod N/R') mod Ns' = o mod Ns', as Ns' divides N/R'
            const uint32_t e = (j2 * r2) << (kNttMaxLog - log_ns2 - next_m);
            v = fr30_mul(v, fr30_mul(fr30_table(hi, e >> 11), fr30_table(lo, e & (kNttTableLen - 1))));
        } else {
            v = fr30_mul(v, last_c);
        }
        uint32_t l[8];
        fr30_to_limbs(v, l);
        uint4* p = reinterpret_cast<uint4*>(out) + 2 * (size_t)o;
        p[0] = make_uint4(l[0], l[1], l[2], l[3]);
        p[1] = make_uint4(l[4], l[5], l[6], l[7]);
    }
}

constexpr uint32_t kNttLdsBytes = kNttTile * kR9 * 4;

}  // namespace

bool ntt_prepare_device() {
    return hipFuncSetAttribute((const void*)k_ntt_pass, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kNttLdsBytes) ==
           hipSuccess;
}

NttPlan ntt_plan(uint32_t log_n) {
    NttPlan p = {};
    if (log_n <= kNttTileLog) {
        p.passes = 1;
        p.m[0] = log_n;
        return p;
    }
    p.passes = (log_n + kNttMaxRadixLog - 1) / kNttMaxRadixLog;
    for (uint32_t i = 0; i < p.passes; i++) p.m[i] = log_n / p.passes + (i < log_n % p.passes ? 1u : 0u);
    return p;
}

void launch_ntt(hipStream_t s, const uint32_t* d_in, uint32_t* d_out, uint32_t log_n, const void* d_tw, const Fr30& last_c,
                uint32_t* d_buf_a, uint32_t* d_buf_b) {
    const NttPlan p = ntt_plan(log_n);
    const uint32_t* src = d_in;
    uint32_t log_ns = 0;
    for (uint32_t i = 0; i < p.passes; i++) {
        uint32_t* dst = i + 1 == p.passes ? d_out : (i % 2 == 0 ? d_buf_a : d_buf_b);
        const uint32_t m = p.m[i];
        const uint32_t log_j = p.passes == 1 ? 0u : kNttTileLog - m;
        const uint32_t blocks = 1u << (log_n - m - log_j);
        const uint32_t lds = (1u << (m + log_j)) * kR9 * 4;
        const uint32_t next_m = i + 1 < p.passes ? p.m[i + 1] : 0u;
        hipLaunchKernelGGL(k_ntt_pass, dim3(blocks), dim3(kNttThreads), lds, s, src, dst, (const Fr30*)d_tw, log_n, m, log_ns,
                           log_j, next_m, last_c);
        src = dst;
        log_ns += m;
    }
}

}  // namespace kzg
