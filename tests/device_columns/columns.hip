// columns.hip -- fq_mul, fq_sqr, fq_mul_sub, fq_mul_minus, fq_mul_plus and fq_sqr_minus of csrc/field30.hip.h as hipcc compiles
// them for the device WITH the switch msm_accum.hip sets (KZG_F30_SERIAL_COLUMNS: every column one multiply-add chain from
// the carry, fq_mul_sub on a negated operand), one WAVE per case: all 64 lanes run the same row and each writes its own
// result.  Test infrastructure only (tests/test_accum_columns_gpu.py loads libkzg_devcolumns.so; tests/device/ builds the
// same header without the switch); nothing here is linked into the library.
// Rows: 52 ints (a, b, c, d: tests/host/field30_columns_host.cpp makes them).  Results: 64 x 13 ints per row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define KZG_F30_SERIAL_COLUMNS 1
#include "field30.hip.h"

using namespace kzg;

namespace {

constexpr int kBlock = 256;
constexpr int kRow = 4 * kQ;

__device__ __forceinline__ Fq ld_fq(const int32_t* p) {
    Fq r;
#pragma unroll
    for (int i = 0; i < kQ; i++) r.d[i] = p[i];
    return r;
}

// (the row index comes from the lane's own thread index: the operands are vector registers, as in the kernel)
template <int kOp>
__global__ void __launch_bounds__(kBlock) k_columns(const int32_t* __restrict__ in, int32_t* __restrict__ out, int n) {
    const int lane = blockIdx.x * kBlock + threadIdx.x;
    const int row = lane >> 6;
    if (row >= n) return;
    const int32_t* r = in + (size_t)row * kRow;
    const Fq a = ld_fq(r), b = ld_fq(r + kQ), c = ld_fq(r + 2 * kQ), d = ld_fq(r + 3 * kQ);
    Fq z;
    if (kOp == 0) z = fq_mul(a, b);
    else if (kOp == 1) z = fq_sqr(a);
    else if (kOp == 2) z = fq_mul_sub(a, b, c, d);
    else if (kOp == 3) z = fq_mul_minus(a, b, c);
    else if (kOp == 4) z = fq_mul_plus(a, b, c);
    else z = fq_sqr_minus(a, c);
    int32_t* o = out + (size_t)lane * kQ;
#pragma unroll
    for (int i = 0; i < kQ; i++) o[i] = z.d[i];
}

struct Buffers {  // device copies of one launch: freed on every path
    int32_t* in = nullptr;
    int32_t* out = nullptr;
    ~Buffers() {
        if (in) (void)hipFree(in);
        if (out) (void)hipFree(out);
    }
};

}  // namespace

// rows: n x 52 ints; out: n x 64 x 13 ints.  Returns the HIP status (0 = success), -1 for a shape the kernels do not take.
extern "C" int devcol_run(int op, const int32_t* rows, int n, int32_t* out) {
    if (op < 0 || op > 5 || n <= 0 || n > 65536) return -1;
    const size_t in_ints = (size_t)n * kRow, out_ints = (size_t)n * 64 * kQ;
    Buffers b;
    hipError_t e = hipMalloc(&b.in, in_ints * 4);
    if (e == hipSuccess) e = hipMalloc(&b.out, out_ints * 4);
    if (e == hipSuccess) e = hipMemcpy(b.in, rows, in_ints * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(b.out, 0x5a, out_ints * 4);  // a result that is not written does not pass for one
    if (e == hipSuccess) {
        const dim3 grid((unsigned)(((size_t)n * 64 + kBlock - 1) / kBlock)), block(kBlock);
        switch (op) {
            case 0: hipLaunchKernelGGL(k_columns<0>, grid, block, 0, 0, b.in, b.out, n); break;
            case 1: hipLaunchKernelGGL(k_columns<1>, grid, block, 0, 0, b.in, b.out, n); break;
            case 2: hipLaunchKernelGGL(k_columns<2>, grid, block, 0, 0, b.in, b.out, n); break;
            case 3: hipLaunchKernelGGL(k_columns<3>, grid, block, 0, 0, b.in, b.out, n); break;
            case 4: hipLaunchKernelGGL(k_columns<4>, grid, block, 0, 0, b.in, b.out, n); break;
            default: hipLaunchKernelGGL(k_columns<5>, grid, block, 0, 0, b.in, b.out, n); break;
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, b.out, out_ints * 4, hipMemcpyDeviceToHost);
    return (int)e;
}
