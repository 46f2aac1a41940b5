// prims.hip -- the field and group-law primitives of csrc as hipcc compiles them for the device, one small kernel and
// one C launcher each.  Test infrastructure only (tests/test_device_prims_gpu.py loads libkzg_devprims.so); nothing here
// is linked into the library.  Records and expectations: tests/prim_cases.py; the per-record bodies: prim_ops.h.
//
// Launchers: (records in, ints per record, results out, ints per result, record count) -> the HIP status as an int
// (0 = success), -1 for a shape the kernel does not take.  One allocation per call, no retries, never an abort.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "prim_ops.h"

using namespace prim;

namespace {

constexpr int kBlock = 256;

struct Buffers {  // device copies of one launch: freed on every path
    int32_t* in = nullptr;
    int32_t* aux = nullptr;
    int32_t* out = nullptr;
    ~Buffers() {
        if (in) (void)hipFree(in);
        if (aux) (void)hipFree(aux);
        if (out) (void)hipFree(out);
    }
};

// stage `in`, run launch(), fetch `out`
template <class Launch>
int run(const int32_t* in, size_t in_ints, int32_t* out, size_t out_ints, Launch launch) {
    Buffers b;
    hipError_t e = hipMalloc(&b.in, in_ints * 4);
    if (e == hipSuccess) e = hipMalloc(&b.out, out_ints * 4);
    if (e == hipSuccess) e = hipMemcpy(b.in, in, in_ints * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(b.out, 0x5a, out_ints * 4);  // a result that is not written does not pass for one
    if (e == hipSuccess) {
        launch(b);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, b.out, out_ints * 4, hipMemcpyDeviceToHost);
    return (int)e;
}

int blocks_for(long lanes) { return (int)((lanes + kBlock - 1) / kBlock); }

}  // namespace

// ---- one lane per record ---------------------------------------------------------------------------------------------------
#define PRIM_ONE_LANE(NAME, IW, OW)                                                                                      \
    __global__ void __launch_bounds__(kBlock) k_##NAME(const int32_t* __restrict__ in, int32_t* __restrict__ out, int n) { \
        const int i = blockIdx.x * kBlock + threadIdx.x;                                                                   \
        if (i >= n) return;                                                                                                \
        pop_##NAME(in + (size_t)i * (IW), out + (size_t)i * (OW));                                                         \
    }                                                                                                                      \
    extern "C" int devprim_##NAME(const int32_t* in, int iw, int32_t* out, int ow, int n) {                                \
        if (iw != (IW) || ow != (OW) || n <= 0) return -1;                                                                 \
        return run(in, (size_t)n * (IW), out, (size_t)n * (OW),                                                \
                   [&](Buffers& b) { hipLaunchKernelGGL(k_##NAME, dim3(blocks_for(n)), dim3(kBlock), 0, 0, b.in, b.out, n); }); \
    }
PRIM_FQ_OPS(PRIM_ONE_LANE)
PRIM_FR_OPS(PRIM_ONE_LANE)

// one lane per BATCH of affine pairs (rows off[b] .. off[b + 1] - 1 share one inversion)
__global__ void __launch_bounds__(kBlock) k_pair_batch(const int32_t* __restrict__ in, const int32_t* __restrict__ off,
                                                       int32_t* __restrict__ out, int32_t* __restrict__ prefix, int nb) {
    const int b = blockIdx.x * kBlock + threadIdx.x;
    if (b >= nb) return;
    pop_pair_batch(in, off[b], off[b + 1], out, prefix);
}
extern "C" int devprim_pair_batch(const int32_t* in, int iw, const int32_t* off, int nb, int32_t* out, int ow, int n) {
    if (iw != 54 || ow != 27 || n <= 0 || nb <= 0 || off[0] != 0 || off[nb] != n) return -1;
    for (int b = 0; b < nb; b++)
        if (off[b] > off[b + 1]) return -1;
    Buffers b;
    hipError_t e = hipMalloc(&b.in, ((size_t)n * 54 + (size_t)nb + 1) * 4);  // rows, then the offsets
    if (e == hipSuccess) e = hipMalloc(&b.aux, (size_t)n * kF * 4);
    if (e == hipSuccess) e = hipMalloc(&b.out, (size_t)n * 27 * 4);
    if (e == hipSuccess) e = hipMemcpy(b.in, in, (size_t)n * 54 * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(b.in + (size_t)n * 54, off, ((size_t)nb + 1) * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(b.out, 0x5a, (size_t)n * 27 * 4);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_pair_batch, dim3(blocks_for(nb)), dim3(kBlock), 0, 0, b.in, b.in + (size_t)n * 54, b.out, b.aux, nb);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, b.out, (size_t)n * 27 * 4, hipMemcpyDeviceToHost);
    return (int)e;
}

// ---- one quad per record: 64 records per workgroup, 16 per wave; every lane writes its own copy of the result ---------------
// Record counts are multiples of 16, so a wave is either whole or absent.
// kBranch: only records whose call flag (word 104) is set make the call, the way KZG_TREE_ADD sits behind `if (l < off)`.
template <bool kBranch>
__global__ void __launch_bounds__(kBlock) k_add_quad(const int32_t* __restrict__ in, int32_t* __restrict__ out, int n) {
    const int c = (blockIdx.x * kBlock + threadIdx.x) >> 2;
    const uint32_t q = threadIdx.x & 3u;
    if (c >= n) return;
    const int32_t* r = in + (size_t)c * 105;
    XYZZ30 acc = ld_xyzz(r);
    const XYZZ30 b = ld_xyzz(r + kX);
    if (kBranch) {
        if (r[2 * kX] != 0) xyzz30_add_quad(acc, b, q);
    } else {
        xyzz30_add_quad(acc, b, q);
    }
    st_xyzz(out + ((size_t)c * 4 + q) * kX, acc);
}
__global__ void __launch_bounds__(kBlock) k_add_quad_dense(const int32_t* __restrict__ in, int32_t* __restrict__ out, int n) {
    const int c = (blockIdx.x * kBlock + threadIdx.x) >> 2;
    const uint32_t q = threadIdx.x & 3u;
    if (c >= n) return;
    const int32_t* r = in + (size_t)c * 105;
    XYZZ30 acc = ld_xyzz(r);
    xyzz30_add_quad_dense(acc, ld_xyzz(r + kX), q);
    st_xyzz(out + ((size_t)c * 4 + q) * kX, acc);
}
// the dense form inside a loop whose trip count (word 208, 0..3) differs from quad to quad, as in k_tree_sum
__global__ void __launch_bounds__(kBlock) k_add_quad_dense_loop(const int32_t* __restrict__ in, int32_t* __restrict__ out, int n) {
    const int c = (blockIdx.x * kBlock + threadIdx.x) >> 2;
    const uint32_t q = threadIdx.x & 3u;
    if (c >= n) return;
    const int32_t* r = in + (size_t)c * 209;
    XYZZ30 acc = ld_xyzz(r);
    int trip = r[(1 + kLoopOps) * kX];
    trip = trip < 0 ? 0 : (trip > kLoopOps ? kLoopOps : trip);
    for (int s = 0; s < trip; s++) {
        const XYZZ30 b = ld_xyzz(r + (1 + s) * kX);
        xyzz30_add_quad_dense(acc, b, q);
    }
    st_xyzz(out + ((size_t)c * 4 + q) * kX, acc);
}
// chains of 16 additions from infinity; every partial sum of every lane is written
template <bool kDense>
__global__ void __launch_bounds__(kBlock) k_chain_quad(const int32_t* __restrict__ in, int32_t* __restrict__ out, int n) {
    const int c = (blockIdx.x * kBlock + threadIdx.x) >> 2;
    const uint32_t q = threadIdx.x & 3u;
    if (c >= n) return;
    XYZZ30 acc = xyzz30_inf();
    for (int s = 0; s < kChain; s++) {
        const XYZZ30 b = ld_xyzz(in + ((size_t)c * kChain + s) * kX);
        if (kDense) xyzz30_add_quad_dense(acc, b, q);
        else xyzz30_add_quad(acc, b, q);
        st_xyzz(out + (((size_t)c * kChain + s) * 4 + q) * kX, acc);
    }
}
#define PRIM_QUAD(NAME, KERNEL, IW, OW)                                                                                    \
    extern "C" int devprim_##NAME(const int32_t* in, int iw, int32_t* out, int ow, int n) {                                  \
        if (iw != (IW) || ow != (OW) || n <= 0 || n % 16 != 0) return -1;                                                    \
        return run(in, (size_t)n * (IW), out, (size_t)n * (OW),                                                  \
                   [&](Buffers& b) { hipLaunchKernelGGL((KERNEL), dim3(blocks_for(4L * n)), dim3(kBlock), 0, 0, b.in, b.out, n); }); \
    }
PRIM_QUAD(add_quad, k_add_quad<false>, 105, 4 * 52)
PRIM_QUAD(add_quad_branch, k_add_quad<true>, 105, 4 * 52)
PRIM_QUAD(add_quad_dense, k_add_quad_dense, 105, 4 * 52)
PRIM_QUAD(add_quad_dense_loop, k_add_quad_dense_loop, 209, 4 * 52)
PRIM_QUAD(chain_quad, k_chain_quad<false>, 16 * 52, 16 * 4 * 52)
PRIM_QUAD(chain_quad_dense, k_chain_quad<true>, 16 * 52, 16 * 4 * 52)

// ---- one step of k_bucket_accumulate's dispatch: one lane per record, whole waves (the record count is a multiple of 64) ----
// A COPY OF THE SHAPE of msm_accum.hip around accum_rare_call, which it has to follow when that changes: the head, the
// wave-uniform ballot branch over the lanes that have a case, the first point of a run read a second time, equal or opposite
// operands (and the pre-test's false positives) through a struct in private memory into ONE real call that hands acc, P and
// Rn back through the same memory, and the tail last, on whatever came back.  (The kernel itself is not shared with this
// file: its code generation stays its own.)  out: the accumulator as it stays in the kernel, then settled.
struct DispatchRare {
    XYZZ30 acc;
    Fq P, Rn;
};
static __device__ __noinline__ bool dispatch_rare_call(DispatchRare* io) { return xyzz30_acc_rare(io->acc, io->P, io->Rn); }
__global__ void __launch_bounds__(kBlock) k_acc_dispatch(const int32_t* __restrict__ in, int32_t* __restrict__ out, int n) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t* r = in + (size_t)i * (kX + 2 * kF + 1);
    const bool neg = r[kX + 2 * kF] != 0;
    XYZZ30 acc = ld_xyzz(r);
    Fq P, Rn;
    uint32_t code;
    {
        const Affine30 p = ld_affine(r + kX);
        code = xyzz30_acc_head(acc, p, neg, P, Rn);
    }
    bool more = code == 0;
    if (__builtin_amdgcn_ballot_w64(code != 0) != 0) {  // (wave-uniform)
        if (code & kAccFresh) {
            if (!(code & kAccPointInf)) {
                const Affine30 p = ld_affine(r + kX);  // read a second time
                xyzz30_acc_set(acc, p, neg);
            }
        } else if (code == kAccMaybeEqual) {
            DispatchRare t;
            t.acc = acc;
            t.P = P;
            t.Rn = Rn;
            more = dispatch_rare_call(&t);
            acc = t.acc;
            P = t.P;
            Rn = t.Rn;
        }
    }
    if (more) xyzz30_acc_tail(acc, P, Rn);
    st_acc_both(out + (size_t)i * 2 * kX, acc);
}

// ---- the quad moves on their own: one lane per record -----------------------------------------------------------------------
// every lane holds its own value v.  out[0..3] = broadcast<SRC>(v) - v: the subtraction right behind the move is the pattern
// that LLVM's DPP combiner folded (g1_30.hip.h); out[4..7] = broadcast<SRC + 1>(v) - broadcast<SRC>(v): both operands moves
// of one register, as P = U2 - U1 and R = S2 - S1 of the cooperative addition are
__global__ void __launch_bounds__(kBlock) k_quad_broadcast(const int32_t* __restrict__ in, int32_t* __restrict__ out, int n) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const Fq v = ld_fq(in + (size_t)i * kF);
    int32_t* o = out + (size_t)i * 8 * kF;
    st_fq(o + 0 * kF, fq_sub_raw(fq_quad_broadcast<0>(v), v));
    st_fq(o + 1 * kF, fq_sub_raw(fq_quad_broadcast<1>(v), v));
    st_fq(o + 2 * kF, fq_sub_raw(fq_quad_broadcast<2>(v), v));
    st_fq(o + 3 * kF, fq_sub_raw(fq_quad_broadcast<3>(v), v));
    const Fq b0 = fq_quad_broadcast<0>(v), b1 = fq_quad_broadcast<1>(v), b2 = fq_quad_broadcast<2>(v), b3 = fq_quad_broadcast<3>(v);
    st_fq(o + 4 * kF, fq_sub_raw(b1, b0));
    st_fq(o + 5 * kF, fq_sub_raw(b2, b1));
    st_fq(o + 6 * kF, fq_sub_raw(b3, b2));
    st_fq(o + 7 * kF, fq_sub_raw(b0, b3));
}
// out = fq_quad_select(lane & 3, a0, a1, a2, a3)
__global__ void __launch_bounds__(kBlock) k_quad_select(const int32_t* __restrict__ in, int32_t* __restrict__ out, int n) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t* r = in + (size_t)i * 4 * kF;
    st_fq(out + (size_t)i * kF, fq_quad_select(threadIdx.x & 3u, ld_fq(r), ld_fq(r + kF), ld_fq(r + 2 * kF), ld_fq(r + 3 * kF)));
}
#define PRIM_LANES64(NAME, IW, OW)                                                                                        \
    extern "C" int devprim_##NAME(const int32_t* in, int iw, int32_t* out, int ow, int n) {                                 \
        if (iw != (IW) || ow != (OW) || n <= 0 || n % 64 != 0) return -1;                                                   \
        return run(in, (size_t)n * (IW), out, (size_t)n * (OW),                                                 \
                   [&](Buffers& b) { hipLaunchKernelGGL(k_##NAME, dim3(blocks_for(n)), dim3(kBlock), 0, 0, b.in, b.out, n); }); \
    }
PRIM_LANES64(acc_dispatch, 79, 104)
PRIM_LANES64(quad_broadcast, 13, 104)
PRIM_LANES64(quad_select, 52, 13)
