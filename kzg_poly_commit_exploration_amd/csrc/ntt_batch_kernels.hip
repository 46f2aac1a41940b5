// ntt_batch_kernels.hip -- the transform of ntt_kernels.hip over a batch of columns (kzg_ntt_batch): every pass of the
// Stockham plan is one launch for the whole batch, blockIdx.y selects the column.  Geometry, arithmetic and twiddle tables
// are k_ntt_pass's (ntt_kernels.hip, DESIGN.md sections 4.6 and 4.25): 256 lanes, tiles of 2^11 values in nine LDS digit
// planes, so that every output column is bit for bit what kzg_ntt gives for that column.
//
// Layout (Stockham autosort, radix 2^m per pass).  Pass p with Ns = product of the earlier radices and R = 2^m reads
// v_r = in[j + r N/R] (r < R) for each j < N/R, computes the R-point DFT of (v_r w_{Ns R}^((j mod Ns) r)), and writes its
// output r to out[(j / Ns) Ns R + (j mod Ns) + r Ns].  The input twiddle of pass p + 1 depends only on the index o that
// pass p writes, so pass p multiplies by it before the store.  The last pass multiplies by a constant instead.
//
// Bounds (fr30.hip.h's conventions).  A loaded value is an integer below 2^256 < 2.3 r (canonical for every pass but the
// first, and for the first whenever the caller respects the ABI).  The first stage of a tile has twiddle 1: |v| < 4.6 r.
// Every later stage adds a product (|w b| <= 0.5001 r + |w b| / 2^270 < 0.5002 r for |b| < 2^259) to one half and
// subtracts it from the other: after m <= 11 stages |v| < 4.6 r + 10 * 0.5002 r < 10 r < 2^259.  Every add / sub is
// carry-normalised (fr30_norm: digits of two normalised operands sum to < 2^30 + 8 < 2^31 - 2^29), so digits 0..7 stay in
// [-2^29 - 4, 2^29 + 4] and the top digit below 2^20: inside fr30_mul's operand bound.  The closing product brings every
// value back to |v| <= 0.5002 r, inside (-r, 2r), which fr30_to_limbs reduces to the canonical residue.
//
// Indices.  Inside a column every index is below N <= 2^22 and stays in 32 bits, as in k_ntt_pass.  The column's offset
// (column x stride values of 8 words) is formed in 64 bits: 64 columns of 2^22 values are 2^31 words.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "fr30.hip.h"
#include "fr30_lanes.hip.h"

namespace kzg {

namespace {

constexpr uint32_t kNttbThreads = 256;

// (the four helpers of ntt_kernels.hip, repeated: that unit's anonymous namespace keeps them to itself)
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

// k_ntt_pass for column blockIdx.y of a batch: the column is at in + 8 blockIdx.y in_stride words and goes to
// out + 8 blockIdx.y out_stride words (strides in values).  Workgroup blockIdx.x takes the tile of J = 2^log_j consecutive j
// and R = 2^m values each (T = J R <= kNttTile).  in and out may be the same buffer with the same stride when a column's
// whole transform is one workgroup (a single pass), so neither is __restrict__: every load of the tile comes before the
// first __syncthreads and every store after the last, and no workgroup touches another column.
__global__ void __launch_bounds__(kNttbThreads) k_nttb_pass(const uint32_t* in, uint64_t in_stride, uint32_t* out, uint64_t out_stride,
                                                            const Fr30* __restrict__ tw, uint32_t log_n, uint32_t m, uint32_t log_ns,
                                                            uint32_t log_j, uint32_t next_m, Fr30 last_c) {
    extern __shared__ int32_t lds[];
    const uint32_t T = 1u << (m + log_j);
    const uint32_t R = 1u << m;
    const uint32_t J = 1u << log_j;
    const uint32_t j0 = blockIdx.x << log_j;
    const Fr30* __restrict__ lo = tw;
    const Fr30* __restrict__ hi = tw + kNttTableLen;
    const uint4* col_in = reinterpret_cast<const uint4*>(in) + 2 * ((uint64_t)blockIdx.y * in_stride);
    uint4* col_out = reinterpret_cast<uint4*>(out) + 2 * ((uint64_t)blockIdx.y * out_stride);

    // load: runs of J consecutive j per r (coalesced), stored at the bit-reversed position of r
    for (uint32_t t = threadIdx.x; t < T; t += kNttbThreads) {
        const uint32_t jj = t & (J - 1), rr = t >> log_j;
        const uint64_t idx = (uint64_t)(j0 + jj) + ((uint64_t)rr << (log_n - m));
        const uint4* p = col_in + 2 * idx;
        const uint4 a = p[0], b = p[1];
        const uint32_t l[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        const uint32_t pos = (jj << m) + (m ? (__brev(rr) >> (32 - m)) : 0u);
        lds_put(lds, T, pos, fr30_from_limbs(l));
    }
    // radix-2 DIT stages in place; stage s pairs positions p0 and p0 + h (h = 2^s) with twiddle w_(2h)^k
    for (uint32_t s = 0; s < m; s++) {
        __syncthreads();
        const uint32_t h = 1u << s;
        for (uint32_t b = threadIdx.x; b < T / 2; b += kNttbThreads) {
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
    for (uint32_t t = threadIdx.x; t < T; t += kNttbThreads) {
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
        uint4* p = col_out + 2 * (uint64_t)o;
        p[0] = make_uint4(l[0], l[1], l[2], l[3]);
        p[1] = make_uint4(l[4], l[5], l[6], l[7]);
    }
}

constexpr uint32_t kNttbLdsBytes = kNttTile * kR9 * 4;

}  // namespace

bool ntt_batch_prepare_device() {
    return hipFuncSetAttribute((const void*)k_nttb_pass, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kNttbLdsBytes) ==
           hipSuccess;
}

void launch_ntt_batch(hipStream_t s, const uint32_t* d_in, uint64_t in_stride, uint32_t* d_out, uint64_t out_stride, uint32_t log_n,
                      uint32_t batch, const void* d_tw, const Fr30& last_c, uint32_t* d_buf_a, uint32_t* d_buf_b) {
    if (!batch) return;
    const NttPlan p = ntt_plan(log_n);
    const uint64_t n = (uint64_t)1 << log_n;
    const uint32_t* src = d_in;
    uint64_t src_stride = in_stride;
    uint32_t log_ns = 0;
    for (uint32_t i = 0; i < p.passes; i++) {
        const bool last = i + 1 == p.passes;
        uint32_t* dst = last ? d_out : (i % 2 == 0 ? d_buf_a : d_buf_b);
        const uint64_t dst_stride = last ? out_stride : n;
        const uint32_t m = p.m[i];
        const uint32_t log_j = p.passes == 1 ? 0u : kNttTileLog - m;
        const uint32_t blocks = 1u << (log_n - m - log_j);
        const uint32_t lds = (1u << (m + log_j)) * kR9 * 4;
        const uint32_t next_m = last ? 0u : p.m[i + 1];
        hipLaunchKernelGGL(k_nttb_pass, dim3(blocks, batch), dim3(kNttbThreads), lds, s, src, src_stride, dst, dst_stride,
                           (const Fr30*)d_tw, log_n, m, log_ns, log_j, next_m, last_c);
        src = dst;
        src_stride = dst_stride;
        log_ns += m;
    }
}

}  // namespace kzg
