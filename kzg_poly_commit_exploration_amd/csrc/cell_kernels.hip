// cell_kernels.hip -- quotients of P by the vanishing polynomials of the cells of a power-of-two domain
// (kzg_cells_and_proofs, kzg_quotient_cells).
//
// Domain of N = 2^K points, cells of l = 2^t.  Cell j is the coset {w_N^(j + (N/l) i) : i < l}; its vanishing polynomial is
// X^l - a_j with a_j = w_N^(j l), and the quotient of P by it is the stride-l synthetic division
//     q_j[i] = c[i + l] + a_j q_j[i + l]        (q_j[i] = 0 for i >= nq = n - l)
// i.e. l independent single-root suffix scans, residue r over the chain i = r, r + l, r + 2l, ... (M = ceil(nq / l) steps).
//
// Lanes.  One lane per (cell p, chunk u, residue r), residue fastest (consecutive lanes read consecutive coefficients),
// chunk u covering chain steps [u Lc, u Lc + Lc).  Two launches, as the single-root scan of poly_kernels.hip:
//   1. k_cells_chunks: the chunk's suffix Horner value with zero carry-in, A_u, to agg[lane] (canonical 8 x u32);
//   2. k_cells_apply: the carry into the chunk, C_u = sum_{v > u} A_v (a_j^Lc)^(v - u - 1), by Horner over the aggregates
//      above it, then the chunk replayed from C_u, every value written to q.  Only a chain's last chunk may be short, and
//      its carry is zero, so a_j^Lc is the right step between every pair of neighbours.
// The host picks Lc ~ sqrt(M) (cells_chunk_log), so a lane's serial work is ~ 2 Lc + U / 2 products (U = M / Lc) however
// long the chain is (l = 1, n = 2^16: Lc = 256, U = 256, ~ 640 products per lane over both launches).
//
// a_j and a_j^Lc come from the context's forward NTT twiddles (ntt_kernels.hip): w_N^e = hi[e' >> 11] * lo[e' & 2047] with
// e' = e 2^(22 - K), already in fr30_mul's multiplier form, so no per-call table is built.
//
// Bounds (fr30.hip.h).  A coefficient and an aggregate are canonical (< r).  A Horner step is fr30_mul(h, a) + x with
// |fr30_mul(h, a)| <= 0.5001 r + |h a| / 2^270 < 0.5002 r (|h| < 2r, |a| < 2^256), so every h stays in (-0.51 r, 1.51 r):
// inside fr30_mul's operand bound after the carry pass and inside (-r, 2r), which fr30_to_limbs reduces to canonical form.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "fr30.hip.h"
#include "fr30_lanes.hip.h"

namespace kzg {

namespace {

constexpr uint32_t kCellThreads = 256;

__device__ __forceinline__ Fr30 cell_horner(const Fr30& h, const Fr30& a, const Fr30& x) {
    return fr30_norm(fr30_add_raw(fr30_mul(h, a), x));
}

struct CellJob {
    const uint32_t* c;  // coefficients, at least nq + l of them
    const Fr30* tw;     // forward NTT twiddles of the context
    uint32_t* agg;      // lanes x 8 words
    uint32_t* q;        // cell p at q + 8 p stride (apply only)
    uint64_t stride;    // scalars between consecutive cells' quotients
    uint64_t lanes;     // polys * U * l
    uint32_t nq;        // quotient length (n' - l)
    uint32_t log_n, log_l, log_lc;
    uint32_t first_cell;
    uint32_t U;         // chunks per chain
};

// lane -> (cell p, chunk u, residue r); the chain steps [k0, k1) of the chunk (empty when k0 >= M_r)
struct CellLane {
    uint32_t p, u, r, k0, k1;
};
__device__ __forceinline__ CellLane cell_lane(const CellJob& J, uint64_t t) {
    CellLane L;
    const uint32_t l = 1u << J.log_l;
    L.r = (uint32_t)t & (l - 1);
    const uint64_t pu = t >> J.log_l;
    L.u = (uint32_t)(pu % J.U);
    L.p = (uint32_t)(pu / J.U);
    const uint32_t m_r = L.r < J.nq ? (J.nq - L.r + l - 1) >> J.log_l : 0u;  // chain steps of residue r
    L.k0 = L.u << J.log_lc;
    const uint32_t end = L.k0 + (1u << J.log_lc);
    L.k1 = end < m_r ? end : m_r;
    if (L.k1 < L.k0) L.k1 = L.k0;
    return L;
}

__global__ void __launch_bounds__(kCellThreads) k_cells_chunks(CellJob J) {
    const uint64_t t = (uint64_t)blockIdx.x * kCellThreads + threadIdx.x;
    if (t >= J.lanes) return;
    const CellLane L = cell_lane(J, t);
    const uint32_t cell = J.first_cell + L.p;
    const Fr30 a = fr30_root(J.tw, cell << J.log_l, J.log_n);  // a_j = w_N^(j l), j l < N
    Fr30 h = fr30_zero();
    for (uint32_t k = L.k1; k-- > L.k0;) h = cell_horner(h, a, fr30_load(J.c + 8 * ((uint64_t)L.r + ((uint64_t)(k + 1) << J.log_l))));
    fr30_store(J.agg + 8 * t, h);
}

__global__ void __launch_bounds__(kCellThreads) k_cells_apply(CellJob J) {
    const uint64_t t = (uint64_t)blockIdx.x * kCellThreads + threadIdx.x;
    if (t >= J.lanes) return;
    const CellLane L = cell_lane(J, t);
    if (L.k0 >= L.k1) return;
    const uint32_t cell = J.first_cell + L.p;
    const uint32_t mask = (1u << J.log_n) - 1u;
    // carry: Horner over the aggregates of the chunks above, step a_j^Lc
    Fr30 h = fr30_zero();
    {
        const Fr30 a_lc = fr30_root(J.tw, (uint32_t)(((uint64_t)cell << (J.log_l + J.log_lc)) & mask), J.log_n);
        const uint64_t row = (uint64_t)L.p * J.U;
        for (uint32_t v = J.U; v-- > L.u + 1;)
            h = cell_horner(h, a_lc, fr30_load(J.agg + 8 * (((row + v) << J.log_l) + L.r)));
    }
    const Fr30 a = fr30_root(J.tw, cell << J.log_l, J.log_n);
    uint32_t* q = J.q + 8 * (uint64_t)L.p * J.stride;
    for (uint32_t k = L.k1; k-- > L.k0;) {
        const uint64_t i = (uint64_t)L.r + ((uint64_t)k << J.log_l);
        h = cell_horner(h, a, fr30_load(J.c + 8 * (i + (1u << J.log_l))));
        fr30_store(q + 8 * i, h);
    }
}

// out[j l + i] = in[j + (N / l) i]: the NTT's natural order gathered into cells
__global__ void __launch_bounds__(kCellThreads) k_cells_gather(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                               uint32_t log_n, uint32_t log_l) {
    const uint32_t o = blockIdx.x * kCellThreads + threadIdx.x;
    if (o >= (1u << log_n)) return;
    const uint32_t j = o >> log_l, i = o & ((1u << log_l) - 1u);
    const uint4* src = reinterpret_cast<const uint4*>(in) + 2 * (size_t)(j + (i << (log_n - log_l)));
    uint4* dst = reinterpret_cast<uint4*>(out) + 2 * (size_t)o;
    dst[0] = src[0];
    dst[1] = src[1];
}

}  // namespace

uint32_t cells_chunk_log(uint32_t nq, uint32_t log_l) {
    const uint32_t m = (nq + (1u << log_l) - 1) >> log_l;
    uint32_t lg = 2;  // at least 4 steps per lane
    while (lg < 16 && ((uint64_t)1 << (2 * lg)) < m) lg++;
    return lg;
}

uint64_t cells_agg_words(uint32_t nq, uint32_t log_l, uint32_t cells) {
    const uint32_t m = (nq + (1u << log_l) - 1) >> log_l;
    const uint32_t lg = cells_chunk_log(nq, log_l);
    const uint64_t U = (m + (1u << lg) - 1) >> lg;
    return (uint64_t)cells * (U ? U : 1) * (1u << log_l) * 8;
}

void launch_cell_quotients(hipStream_t s, const uint32_t* d_coeffs, uint32_t nq, uint32_t log_n, uint32_t log_l,
                           uint32_t first_cell, uint32_t cells, const void* d_tw, uint32_t* d_agg, uint32_t* d_q,
                           uint64_t stride) {
    if (!nq || !cells) return;
    CellJob J;
    J.c = d_coeffs;
    J.tw = (const Fr30*)d_tw;
    J.agg = d_agg;
    J.q = d_q;
    J.stride = stride;
    J.nq = nq;
    J.log_n = log_n;
    J.log_l = log_l;
    J.log_lc = cells_chunk_log(nq, log_l);
    J.first_cell = first_cell;
    const uint32_t m = (nq + (1u << log_l) - 1) >> log_l;
    J.U = (m + (1u << J.log_lc) - 1) >> J.log_lc;
    J.lanes = (uint64_t)cells * J.U << log_l;
    const dim3 grid((unsigned)((J.lanes + kCellThreads - 1) / kCellThreads));
    hipLaunchKernelGGL(k_cells_chunks, grid, dim3(kCellThreads), 0, s, J);
    hipLaunchKernelGGL(k_cells_apply, grid, dim3(kCellThreads), 0, s, J);
}

void launch_cells_gather(hipStream_t s, const uint32_t* d_evals, uint32_t* d_out, uint32_t log_n, uint32_t log_l) {
    const uint32_t N = 1u << log_n;
    hipLaunchKernelGGL(k_cells_gather, dim3((N + kCellThreads - 1) / kCellThreads), dim3(kCellThreads), 0, s, d_evals, d_out,
                       log_n, log_l);
}

}  // namespace kzg
