// srs_io.hip -- SRS ingestion from the wire / on-disk forms, on the device:
//  * affine points (x, y as blst_fp, 96 bytes): what the binary cache of kzg_srs_save holds -- no normalisation;
//  * compressed points (48 bytes, ZCash encoding: reference src/curves.rs:99-183, the strings of the CLI's
//    setup.json): every lane decompresses one point, y = (x^3 + 4)^((p+1)/4) with the sign bit of the encoding,
//    instead of one blst_p1_uncompress per point on the host.
// Both write table level 0 in the table's own record form (x digits in words 0..12, y digits in words 16..28 of a 128-byte
// record, all zero = infinity); srs_kernels.hip builds the other levels from it.
#include "engine.h"
#include "field30.hip.h"
#include "wire30.hip.h"

namespace kzg {

// 96-byte affine records (x, y as blst_fp: 12 x u32, Montgomery R = 2^384) -> 128-byte table records; (0, 0) = infinity
__global__ void __launch_bounds__(256) k_affine96_to_table(const uint4* __restrict__ in, uint32_t n, uint4* __restrict__ table) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint4* src = in + (size_t)i * 6;
    uint4* dst = table + (size_t)i * kAffineU4;
    uint32_t w[24];
#pragma unroll
    for (int t = 0; t < 6; t++) {
        const uint4 v = src[t];
        w[4 * t] = v.x; w[4 * t + 1] = v.y; w[4 * t + 2] = v.z; w[4 * t + 3] = v.w;
    }
    uint32_t any = 0;
#pragma unroll
    for (int t = 0; t < 24; t++) any |= w[t];
    if (!any) {
        const uint4 zero = make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 8; t++) dst[t] = zero;
        return;
    }
    // stored s = x * 2^384; the signed form wants x * 2^390 = 64 s: the same bits six places higher, then one product
    // with the Montgomery one to bring the magnitude below 0.62 p
    store_digits16(dst, fq_mul(fq_from_u32x12(w), fq_one()));
    store_digits16(dst + 4, fq_mul(fq_from_u32x12(w + 12), fq_one()));
}

// status[0]: index + 1 of the first malformed point (0 = all good), by atomicMin on index + 1 (pre-set to 0xffffffff).
// The decoder is wire30.hip.h's (the verifiers' byte-string entry points run the same one, wire_kernels.hip).
__global__ void __launch_bounds__(64) k_uncompress(const uint4* __restrict__ in, uint32_t n, uint4* __restrict__ table,
                                                   uint32_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    uint4* dst = table + (size_t)i * kAffineU4;
    uint32_t raw[12];
    load_wire48(in + (size_t)i * 3, raw);
    Fq x, y;
    const uint32_t st = wire_g1_decode(raw, x, y);
    store_digits16(dst, x);
    store_digits16(dst + 4, y);
    if (st & kWireBad) atomicMin(status, i + 1);
}

void launch_affine96_to_table(hipStream_t s, const void* d_affine96, uint32_t n, void* d_table) {
    if (!n) return;
    hipLaunchKernelGGL(k_affine96_to_table, dim3((n + 255) / 256), dim3(256), 0, s, (const uint4*)d_affine96, n, (uint4*)d_table);
}
void launch_uncompress(hipStream_t s, const void* d_compressed, uint32_t n, void* d_table, uint32_t* d_status) {
    if (!n) return;
    hipLaunchKernelGGL(k_uncompress, dim3((n + 63) / 64), dim3(64), 0, s, (const uint4*)d_compressed, n, (uint4*)d_table, d_status);
}

}  // namespace kzg
