// blob_kernels.hip -- outputs of the producing side encoded on the device into the bytes they travel as (DESIGN.md section
// 4.13), the mirror of wire_kernels.hip: one lane per G1 point, one lane per scalar, the encoders of wire_enc30.hip.h.
//   k_enc_g1     the 128-byte affine record (all zero = infinity) -> 48 compressed bytes; with bit_reversed, record j of
//                every row of 2^log_row records goes to slot brp(j) of the row (a row: the proofs of one polynomial, so that
//                slot c holds the proof of this API's cell brp(c))
//   k_enc_fr     a blst_fr image -> 32 big-endian bytes; with bit_reversed, value i of cell j goes to position brp(i) of cell
//                brp(j), cells of 2^log_row values, 2^log_cells cells per polynomial (k_wire_fr's permutation backwards, and
//                the permutation of whole cells)
//   k_poly_trim  per polynomial, 1 + the index of its highest non-zero coefficient (0 for the zero polynomial): atomicMax
//                into one word per polynomial, pre-set to zero; the same pass multiplies the coefficients by the 1 / n that
//                the unnormalised inverse DFT in front of it left out
// k_enc_fr's launch has one error word, pre-set to 0xffffffff: atomicMin of the least source index whose image is not below r.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "wire_enc30.hip.h"

namespace kzg {

namespace {
constexpr uint32_t kEncG1Threads = 64;
constexpr uint32_t kEncFrThreads = 256;
constexpr uint32_t kTrimThreads = 256;

__device__ __forceinline__ Fq load_digits16(const uint4* __restrict__ p) {
    const uint4 a = p[0], b = p[1], c = p[2], d = p[3];
    Fq r;
    r.d[0] = (int32_t)a.x; r.d[1] = (int32_t)a.y; r.d[2] = (int32_t)a.z; r.d[3] = (int32_t)a.w;
    r.d[4] = (int32_t)b.x; r.d[5] = (int32_t)b.y; r.d[6] = (int32_t)b.z; r.d[7] = (int32_t)b.w;
    r.d[8] = (int32_t)c.x; r.d[9] = (int32_t)c.y; r.d[10] = (int32_t)c.z; r.d[11] = (int32_t)c.w;
    r.d[12] = (int32_t)d.x;
    return r;
}
}  // namespace

__global__ void __launch_bounds__(kEncG1Threads) k_enc_g1(const uint4* __restrict__ in, uint32_t n, uint32_t log_row,
                                                          uint32_t bit_reversed, uint4* __restrict__ out) {
    const uint32_t i = blockIdx.x * kEncG1Threads + threadIdx.x;
    if (i >= n) return;
    const uint4* src = in + (size_t)i * kAffineU4;
    const Fq x = load_digits16(src), y = load_digits16(src + 4);
    uint32_t raw[12];
    wire_g1_encode(x, y, raw);
    const uint32_t mask = (1u << log_row) - 1u;
    const uint32_t pos = bit_reversed ? (i & ~mask) | wire_brp(i & mask, log_row) : i;
    uint4* dst = out + (size_t)pos * 3;
    dst[0] = make_uint4(raw[0], raw[1], raw[2], raw[3]);
    dst[1] = make_uint4(raw[4], raw[5], raw[6], raw[7]);
    dst[2] = make_uint4(raw[8], raw[9], raw[10], raw[11]);
}

__global__ void __launch_bounds__(kEncFrThreads) k_enc_fr(const uint4* __restrict__ in, uint32_t n, uint32_t log_row,
                                                          uint32_t log_cells, uint32_t bit_reversed, uint4* __restrict__ out,
                                                          uint32_t* __restrict__ err) {
    const uint32_t g = blockIdx.x * kEncFrThreads + threadIdx.x;
    if (g >= n) return;
    const uint4 a = in[(size_t)g * 2], b = in[(size_t)g * 2 + 1];
    const uint32_t l[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t raw[8];
    if (wire_fr_encode(l, raw) & kWireBad) atomicMin(err, g);
    const uint32_t rmask = (1u << log_row) - 1u, cmask = (1u << log_cells) - 1u;
    const uint32_t cell = (g >> log_row) & cmask;
    const uint32_t pos = bit_reversed ? (g & ~((cmask << log_row) | rmask)) | (wire_brp(cell, log_cells) << log_row) |
                                            wire_brp(g & rmask, log_row)
                                      : g;
    uint4* dst = out + (size_t)pos * 2;
    dst[0] = make_uint4(raw[0], raw[1], raw[2], raw[3]);
    dst[1] = make_uint4(raw[4], raw[5], raw[6], raw[7]);
}

// grid: (ceil(n / kTrimThreads), batch); polynomial b at io + 2 b stride (uint4 units of 16 bytes, 2 per coefficient).  With
// scale, every coefficient is first multiplied by c (multiplier form: the 1 / n an unnormalised inverse DFT still owes) and
// written back canonical: one pass over the coefficients serves both.
__global__ void __launch_bounds__(kTrimThreads) k_poly_trim(uint4* __restrict__ io, uint32_t n, uint64_t stride, uint32_t scale,
                                                            Fr30 c, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * kTrimThreads + threadIdx.x;
    bool nz = false;
    if (i < n) {
        uint4* p = io + ((size_t)blockIdx.y * stride + i) * 2;
        const uint4 a = p[0], b = p[1];
        // testing the words is testing the value: launch_fr_dft and the recovery kernels write canonical images (below r, so
        // zero has the one image of all-zero words); c is not zero, so the product is zero exactly when the value is
        nz = (a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w) != 0;
        if (scale && nz) {
            const uint32_t l[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            uint32_t o[8];
            fr30_to_limbs(fr30_mul(fr30_from_limbs(l), c), o);
            p[0] = make_uint4(o[0], o[1], o[2], o[3]);
            p[1] = make_uint4(o[4], o[5], o[6], o[7]);
        }
    }
    // one atomic per wave: the highest lane that holds a non-zero coefficient
    const uint64_t m = __ballot(nz);
    if (m && (threadIdx.x & 63u) == 63u - (uint32_t)__clzll((long long)m)) atomicMax(out + blockIdx.y, i + 1);
}

void launch_enc_g1(hipStream_t s, const void* d_affine, uint32_t n, uint32_t log_row, bool bit_reversed, void* d_out48) {
    if (!n) return;
    hipLaunchKernelGGL(k_enc_g1, dim3((n + kEncG1Threads - 1) / kEncG1Threads), dim3(kEncG1Threads), 0, s, (const uint4*)d_affine, n,
                       log_row, bit_reversed ? 1u : 0u, (uint4*)d_out48);
}

void launch_enc_fr(hipStream_t s, const void* d_in, uint32_t n, uint32_t log_row, uint32_t log_cells, bool bit_reversed, void* d_out32,
                   uint32_t* d_err) {
    if (!n) return;
    hipLaunchKernelGGL(k_enc_fr, dim3((n + kEncFrThreads - 1) / kEncFrThreads), dim3(kEncFrThreads), 0, s, (const uint4*)d_in, n, log_row,
                       log_cells, bit_reversed ? 1u : 0u, (uint4*)d_out32, d_err);
}

void launch_poly_trim(hipStream_t s, void* d_coeffs, uint32_t n, uint64_t stride, uint32_t batch, const Fr30* scale, uint32_t* d_out) {
    if (!n || !batch) return;
    hipLaunchKernelGGL(k_poly_trim, dim3((n + kTrimThreads - 1) / kTrimThreads, batch), dim3(kTrimThreads), 0, s, (uint4*)d_coeffs, n,
                       stride, scale ? 1u : 0u, scale ? *scale : fr30_zero(), d_out);
}

}  // namespace kzg
