// wire_kernels.hip -- inputs of the batch verifiers decoded on the device from the bytes they travel as (DESIGN.md section
// 4.12): one lane per compressed G1 point, one lane per 32-byte big-endian scalar, the decoders of wire30.hip.h.
//   k_wire_g1   48 bytes -> the 128-byte affine record k_vc_ladder reads (all zero = infinity), at a record stride of the
//               caller's choosing and optionally gathered through a source-index array
//   k_wire_fr   32 bytes -> the blst_fr image the Fr kernels read; value i of a row of 2^log_row values goes to position
//               brp(i) of the row when the input is in the sampling specs' bit-reversed order (a row: a cell, or a blob)
// Each launch has one error word, pre-set to 0xffffffff: atomicMin of the least input index that did not decode, so that the
// host can name the record, the commitment or the value.  A point that did not decode is written as infinity, a scalar as its
// residue: what follows on the stream stays inside the kernels' contracts, and the host discards the call's result.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "wire30.hip.h"

namespace kzg {

namespace {
constexpr uint32_t kWireG1Threads = 64;
constexpr uint32_t kWireFrThreads = 256;
}  // namespace

__global__ void __launch_bounds__(kWireG1Threads) k_wire_g1(const uint4* __restrict__ in, const uint32_t* __restrict__ src, uint32_t n,
                                                            uint4* __restrict__ out, uint32_t stride_u4, uint32_t* __restrict__ err) {
    const uint32_t i = blockIdx.x * kWireG1Threads + threadIdx.x;
    if (i >= n) return;
    const uint32_t idx = src ? src[i] : i;
    uint32_t raw[12];
    load_wire48(in + (size_t)idx * 3, raw);
    Fq x, y;
    const uint32_t st = wire_g1_decode(raw, x, y);
    if (st & kWireBad) {
        x = fq_zero();
        y = fq_zero();
        atomicMin(err, idx);
    }
    uint4* dst = out + (size_t)i * stride_u4;
    store_digits16(dst, x);
    store_digits16(dst + 4, y);
}

__global__ void __launch_bounds__(kWireFrThreads) k_wire_fr(const uint4* __restrict__ in, uint32_t n, uint32_t log_row,
                                                            uint32_t bit_reversed, uint4* __restrict__ out, uint32_t* __restrict__ err) {
    const uint32_t g = blockIdx.x * kWireFrThreads + threadIdx.x;
    if (g >= n) return;
    uint32_t raw[8], l[8];
    load_wire32(in + (size_t)g * 2, raw);
    if (wire_fr_decode(raw, l) & kWireBad) atomicMin(err, g);
    const uint32_t mask = (1u << log_row) - 1u;
    const uint32_t pos = bit_reversed ? (g & ~mask) | wire_brp(g & mask, log_row) : g;
    uint4* dst = out + (size_t)pos * 2;
    dst[0] = make_uint4(l[0], l[1], l[2], l[3]);
    dst[1] = make_uint4(l[4], l[5], l[6], l[7]);
}

void launch_wire_g1(hipStream_t s, const void* d_in48, const uint32_t* d_src, uint32_t n, void* d_records, uint32_t stride_bytes,
                    uint32_t* d_err) {
    if (!n) return;
    hipLaunchKernelGGL(k_wire_g1, dim3((n + kWireG1Threads - 1) / kWireG1Threads), dim3(kWireG1Threads), 0, s, (const uint4*)d_in48,
                       d_src, n, (uint4*)d_records, stride_bytes / 16, d_err);
}

void launch_wire_fr(hipStream_t s, const void* d_in32, uint32_t n, uint32_t log_row, bool bit_reversed, void* d_out, uint32_t* d_err) {
    if (!n) return;
    hipLaunchKernelGGL(k_wire_fr, dim3((n + kWireFrThreads - 1) / kWireFrThreads), dim3(kWireFrThreads), 0, s, (const uint4*)d_in32, n,
                       log_row, bit_reversed ? 1u : 0u, (uint4*)d_out, d_err);
}

}  // namespace kzg
